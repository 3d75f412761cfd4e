// hgym_net.hip -- actor/critic forward, PPO loss + hand-written backward, grad-norm clip + Adam
// (SURVEY.md §8a rows A1, A2, A8, A10, A11).  All dense products go through gemm_nt_kernel (hgym_gemm.hpp);
// everything else here is the HBM-bound glue: operand packing / transposes, the per-sample Gaussian / PPO
// arithmetic, reductions, the optimiser.
//
// Memory plan (caller-allocated workspace, zero-filled once; layout from ws_layout()):
//   per layer l of each net:  Wp  [N16][Kp]   operand-precision copy of W (rows padded to 16, K to a stage)
//                             WTp [K16][Ncp]  operand-precision copy of W^T (for dX = dY * W)
//   per layer input:          X   [maxM][Kp]  row-major activations (X0 = packed observations)
//                             XT  [K16][Mp]   their transposes (for dW = dY^T * X), update path only
//   per layer output grad:    dY  [maxM][Ncp] and dYT [N16][Mp]
//   split-K slabs             [splits][P] fp32, loss partial sums, scalar outputs
// Pad rows/columns are never written with non-zero data, so zero-fill at allocation keeps every padded
// contraction exact.
#include <stdlib.h>

#include "hgym_gemm.hpp"
#include "hgym_fused.hpp"
#include "hgym_norm.hpp"
#include "hgym_loss.hpp"

namespace hgym {

// ------------------------------------------------------------------------------------------------ layouts
struct LayerLayout {
    int K, N;                // in, out features
    int Kp, Ncp, N16, K16;   // padded sizes (see above)
    int64_t w_off, b_off;    // offsets (floats) into the flat fp32 parameter vector
    int64_t Wp, WTp;         // byte offsets into the workspace
    int64_t X, XT, dY, dYT;  // byte offsets: layer input, its transpose, output grad, its transpose
    // fused bf16 path (hgym_fused.hpp): fragment-major operand copies
    int KBf, NBf, NBBf;      // forward k-blocks of 32, output blocks of 16, backward contraction blocks of 32
    int KRf;                 // forward k-blocks that hold a valid column, ceil(K / 32): what the first-layer loops run (l0_ksteps); KBf sizes every buffer
    int64_t Wf, WTf;         // byte offsets
};

struct NetLayout {
    int L;
    bool fused;              // the fused bf16 layout (fragment-major weights, block-layout activations); else the layer-by-layer one
    LayerLayout layer[HGYM_MAX_LAYERS];
    int64_t out_f32;         // [maxM][N_last] fp32 output of the last layer (update path)
    int64_t X0b, Hb[3], dZb[4];   // fused path: block-layout activations / pre-activation gradients
};

struct WsLayout {
    int es;                  // operand element size
    int SE;                  // stage elements (contraction padding unit)
    int64_t maxM, Mp;        // max batch and its contraction padding (row stride of every transposed buffer)
    int64_t P;               // total parameters
    int64_t Ps;              // slab stride (P rounded up so every slab starts 256-byte aligned)
    NetLayout net[3];        // 0 actor, 1 critic (both fused or neither), 2 auxiliary head (optional; fused only with the other two)
    int nnets;               // 2 or 3
    int64_t aux_p0;          // first parameter of the auxiliary head in the flat vector (= P when absent)
    int splits;
    int64_t slabs;           // [splits][P] fp32
    int64_t partials;        // [MAX_LOSS_BLOCKS][16] fp32
    int64_t zeros;           // 4 KiB that nothing ever writes (the workspace arrives zero-filled)
    int64_t sqn;             // [SQN_BLOCKS] fp64 per-workgroup sums of sqnorm_prologue_kernel + its arrival counter (zero between launches)
    int64_t sigma;           // HGYM_STD_LOG: [SIGMA_FLOATS] fp32, sigma[j] = exp(params[j]) for j < A (sigma_of; adam_kernel and
                             // sync_shadow_kernel keep it current); -1 in HGYM_STD_SCALAR, where the parameters are sigma and nothing is taken
    int64_t total_bytes;
    Act act;                 // the hidden layers' activation (HgymNetConfig.activation, resolved)
    int64_t Mpad;            // fused path: batch padded to the 64-row tile
    int dw_splits;
};

constexpr int MAX_LOSS_BLOCKS = 8192;   // 256 samples each: minibatches up to 2 M samples
constexpr int SQN_BLOCKS = 256;         // workgroups of sqnorm_prologue_kernel
constexpr int RSN_X = 96;               // workgroups per segment of reduce_slabs_kernel
constexpr int SIGMA_FLOATS = 16;        // the derived sigma block (log mode): num_actions <= 12 entries, padded to 64 bytes

// the hidden widths the fused kernels are instantiated for, and the update's tile fits (hgym_fused.hpp: fb_lds_bytes)
static bool fused_trunk_ok(const int32_t* d) {
    if (!(d[1] == 256 || d[1] == 512 || d[1] == 768)) return false;
    if (d[2] % 128 || d[2] > 768 || d[3] % 128 || d[3] > 768) return false;
    return (size_t)fb_lds_bytes(d) <= FB_LDS_LIMIT;
}
static bool fused_supported(const HgymNetConfig* c) {
    if (c->precision != HGYM_BF16 || c->actor_layers != 4 || c->critic_layers != 4) return false;
    if (getenv("HGYM_NO_FUSED")) return false;
    return fused_trunk_ok(c->actor_dims) && c->actor_dims[4] <= 16 && fused_trunk_ok(c->critic_dims) && c->critic_dims[4] <= 16;
}
// the auxiliary head through the fused kernels: head up to 96 columns (three 32-wide contraction blocks), first width 512 (the
// wide-head instantiation of the forward exists for this first width only)
static bool fused_aux_supported(const HgymNetConfig* c) {
    if (c->aux_layers != 4 || getenv("HGYM_NO_FUSED_AUX")) return false;
    const int32_t* d = c->aux_dims;
    return d[1] == 512 && d[4] > 16 && d[4] <= 96 && fused_trunk_ok(d);
}
constexpr int MAX_SPLITS = 32;

// HgymNetConfig.activation / act_alpha / act_scale -> struct Act (hgym_gemm.hpp): defaults filled in, SELU as the ELU form.
// Refuses what the derivative-from-y design cannot carry.
static int32_t act_resolve(const HgymNetConfig* c, Act* a) {
    memset(a, 0, sizeof(*a));
    const int k = c->activation;
    const float al = c->act_alpha, sc = c->act_scale;
    HG_REQUIRE(k >= HGYM_ACT_ELU && k <= HGYM_ACT_SIGMOID, HGYM_E_UNSUPPORTED,
               "activation=%d: not one of HGYM_ACT_ELU, _SELU, _LEAKY_RELU, _TANH, _SIGMOID", k);
    // (written so that a NaN fails it)
    HG_REQUIRE(al >= 0.0f && al < INFINITY && sc >= 0.0f && sc < INFINITY, HGYM_E_BADARG,
               "activation %d: act_alpha=%g, act_scale=%g must be finite and >= 0 (a negative alpha, slope or scale would break "
               "sign(f(z)) = sign(z), from which the backward takes the derivative)", k, al, sc);
    a->kind = k;
    if (k == HGYM_ACT_ELU || k == HGYM_ACT_SELU) {
        a->kind = HGYM_ACT_ELU;
        a->alpha = al != 0.0f ? al : (k == HGYM_ACT_SELU ? 1.6732632423543772f : 1.0f);
        a->scale = sc != 0.0f ? sc : (k == HGYM_ACT_SELU ? 1.0507009873554805f : 1.0f);
        a->d0p = a->scale;
        a->d0n = a->scale * a->alpha;
        a->d1n = 1.0f;
        return HGYM_OK;
    }
    HG_REQUIRE(sc == 0.0f, HGYM_E_BADARG, "activation %d: act_scale=%g is used by ELU / SELU only and must be 0", k, sc);
    HG_REQUIRE(k == HGYM_ACT_LEAKY_RELU || al == 0.0f, HGYM_E_BADARG, "activation %d: act_alpha=%g is not used by Tanh / Sigmoid and must be 0",
               k, al);
    a->alpha = al;
    if (k == HGYM_ACT_LEAKY_RELU) {
        a->d0p = 1.0f;
        a->d0n = al;
    } else {
        a->dq = 1.0f;
        a->d0p = a->d0n = k == HGYM_ACT_TANH ? 1.0f : 0.0f;
        a->d1p = a->d1n = k == HGYM_ACT_TANH ? 0.0f : 1.0f;
    }
    return HGYM_OK;
}

static int32_t ws_layout(const HgymNetConfig* c, WsLayout* w) {
    HG_REQUIRE(c, HGYM_E_BADARG, "null net config");
    HG_REQUIRE(c->precision == HGYM_F32 || c->precision == HGYM_BF16, HGYM_E_BADARG, "precision=%d", c->precision);
    HG_REQUIRE(c->actor_layers >= 1 && c->actor_layers <= HGYM_MAX_LAYERS && c->critic_layers >= 1 &&
                   c->critic_layers <= HGYM_MAX_LAYERS, HGYM_E_SHAPE, "layer counts %d/%d", c->actor_layers, c->critic_layers);
    HG_REQUIRE(c->max_batch > 0, HGYM_E_SHAPE, "max_batch=%d", c->max_batch);
    HG_REQUIRE(c->actor_dims[0] == c->num_obs && c->critic_dims[0] == c->num_priv &&
                   c->actor_dims[c->actor_layers] == c->num_actions && c->critic_dims[c->critic_layers] == 1,
               HGYM_E_SHAPE, "layer dims inconsistent with num_obs/num_priv/num_actions");
    HG_REQUIRE(c->num_actions >= 1 && c->num_actions <= 12, HGYM_E_UNSUPPORTED, "num_actions=%d (loss kernel reduces <=12 per-action sums)",
               c->num_actions);
    memset(w, 0, sizeof(*w));
    const int32_t rc_act = act_resolve(c, &w->act);
    if (rc_act) return rc_act;
    w->es = c->precision == HGYM_F32 ? 4 : 2;
    w->SE = c->precision == HGYM_F32 ? stage_elems<float>() : stage_elems<__bf16>();
    w->maxM = c->max_batch;
    w->Mp = round_up(c->max_batch, w->SE);
    HG_REQUIRE(c->fused_activation == 0 || c->fused_activation == 1, HGYM_E_BADARG,
               "HgymNetConfig.fused_activation=%d (0: the fused bf16 kernels for ELU(1) only, 1: for any activation)", c->fused_activation);
    HG_REQUIRE(c->std_param == HGYM_STD_SCALAR || c->std_param == HGYM_STD_LOG, HGYM_E_BADARG,
               "HgymNetConfig.std_param=%d (HGYM_STD_SCALAR = 0: the parameters hold sigma, HGYM_STD_LOG = 1: log sigma)", c->std_param);
    const bool fused = fused_supported(c) && (act_is_elu1(w->act) || c->fused_activation == 1);
    w->Mpad = round_up(c->max_batch, 64);
    int64_t off = 0, poff = c->num_actions;  // std first (state_dict order)
    auto take = [&](int64_t bytes) {
        const int64_t o = off;
        off += round_up(bytes, 256);
        return o;
    };
    HG_REQUIRE(c->aux_layers >= 0 && c->aux_layers <= HGYM_MAX_LAYERS, HGYM_E_SHAPE, "aux_layers=%d", c->aux_layers);
    if (c->aux_layers > 0) {
        // (SegTable holds 2 x 16 layer segments + std)
        HG_REQUIRE(c->actor_layers + c->critic_layers + c->aux_layers <= 16, HGYM_E_SHAPE,
                   "auxiliary head: %d actor + %d critic + %d auxiliary layers exceed 16 in total", c->actor_layers, c->critic_layers,
                   c->aux_layers);
        HG_REQUIRE(c->aux_dims[0] == c->num_obs, HGYM_E_SHAPE, "auxiliary head: input width %d must be num_obs = %d", c->aux_dims[0],
                   c->num_obs);
        HG_REQUIRE(c->aux_target_offset >= 0 && c->aux_target_offset + c->aux_dims[c->aux_layers] <= c->num_priv, HGYM_E_SHAPE,
                   "auxiliary head: targets [%d, %d) must lie inside the privileged row of %d", c->aux_target_offset,
                   c->aux_target_offset + c->aux_dims[c->aux_layers], c->num_priv);
    }
    w->nnets = c->aux_layers > 0 ? 3 : 2;
    w->aux_p0 = -1;
    for (int which = 0; which < w->nnets; ++which) {
        NetLayout& n = w->net[which];
        n.L = which == 0 ? c->actor_layers : (which == 1 ? c->critic_layers : c->aux_layers);
        const int32_t* dims = which == 0 ? c->actor_dims : (which == 1 ? c->critic_dims : c->aux_dims);
        n.fused = fused && (which < 2 || fused_aux_supported(c));
        if (which == 2) w->aux_p0 = poff;
        for (int l = 0; l < n.L; ++l) {
            LayerLayout& y = n.layer[l];
            y.K = dims[l];
            y.N = dims[l + 1];
            HG_REQUIRE(y.K > 0 && y.N > 0, HGYM_E_SHAPE, "%s layer %d: non-positive layer dim %d -> %d", which == 0 ? "actor" : (which == 1 ? "critic" : "auxiliary"), l, y.K, y.N);
            y.Kp = (int)round_up(y.K, w->SE);
            y.Ncp = (int)round_up(y.N, w->SE);
            y.N16 = (int)round_up(y.N, 16);
            y.K16 = (int)round_up(y.K, 16);
            y.w_off = poff;
            poff += (int64_t)y.N * y.K;
            y.b_off = poff;
            poff += y.N;
            if (n.fused) {
                y.KBf = l == 0 ? l0_ksteps(y.K).KB : (int)round_up(y.K, 32) / 32;      // first layer: whole 128-column chunks
                y.KRf = l == 0 ? l0_ksteps(y.K).KR : y.KBf;
                y.NBf = y.N16 / 16;
                y.NBBf = (int)round_up(y.N, 32) / 32;
                y.Wf = take((int64_t)y.NBf * y.KBf * 1024);
                y.WTf = take((int64_t)y.K16 / 16 * y.NBBf * 1024);
            } else {
                y.Wp = take((int64_t)y.N16 * y.Kp * w->es);
                y.WTp = take((int64_t)y.K16 * y.Ncp * w->es);
                y.X = take(w->maxM * y.Kp * w->es);
                y.XT = take((int64_t)y.K16 * w->Mp * w->es);
                y.dY = take(w->maxM * y.Ncp * w->es);
                y.dYT = take((int64_t)y.N16 * w->Mp * w->es);
            }
        }
        n.out_f32 = take(w->maxM * (int64_t)dims[n.L] * 4);
        if (n.fused) {
            n.X0b = take(w->Mpad * (int64_t)n.layer[0].KBf * 32 * 2);
            for (int l = 0; l < 3; ++l) {
                n.Hb[l] = take(w->Mpad * (int64_t)n.layer[l].N * 2);
                n.dZb[l] = take(w->Mpad * (int64_t)n.layer[l].N * 2);
            }
            n.dZb[3] = take(w->Mpad * 32 * n.layer[3].NBBf * 2);
        }
    }
    w->P = poff;
    if (w->aux_p0 < 0) w->aux_p0 = poff;
    w->Ps = round_up(poff, 64);
    w->splits = MAX_SPLITS;
    w->dw_splits = 8;        // batch splits of the dW contraction, one per XCD (16 measured 3 % slower: twice the slab traffic)
    w->slabs = take((int64_t)w->splits * w->Ps * 4);
    w->partials = take((int64_t)MAX_LOSS_BLOCKS * LOSS_PARTIALS * 4);
    w->zeros = take(4096);
    w->sqn = take((SQN_BLOCKS + 2) * 8);
    w->sigma = c->std_param == HGYM_STD_LOG ? take(SIGMA_FLOATS * 4) : -1;     // behind everything else: no other offset moves
    w->total_bytes = off;
    return HGYM_OK;
}

// ------------------------------------------------------------------------------------------------ small kernels
__global__ __launch_bounds__(1024) void fin_only_kernel(const FinArgs f) { fin_block(f, threadIdx.x, blockDim.x); }

// dst[m][k] = T(src[row(m)][k]) for k < K; row(m) = idx ? idx[m] : m.  Pad columns are left untouched (zero).
template <typename T>
__global__ __launch_bounds__(256) void pack_rows_kernel(int M, int K, const float* __restrict__ src, int64_t ld_src,
                                                        const int64_t* __restrict__ idx, T* __restrict__ dst, int64_t ld_dst) {
    const int64_t total = (int64_t)M * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / K), k = (int)(i - (int64_t)m * K);
        const int64_t r = idx ? idx[m] : m;
        dst[(int64_t)m * ld_dst + k] = from_f32<T>(src[r * ld_src + k]);
    }
}

// out[c][m] = in[m][c] for c < C, m < M; out[c][m] = 0 for M <= m < Mp  (Mp = contraction padding of this call)
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(int M, int Mp, int C, const T* __restrict__ in, int64_t ld_in,
                                                        T* __restrict__ out, int64_t ld_out) {
    __shared__ T tile[64][66];
    const int m0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 4 row groups
    for (int r = ty; r < 64; r += 4) {
        const int m = m0 + r, c = c0 + tx;
        tile[r][tx] = (m < M && c < C) ? in[(int64_t)m * ld_in + c] : from_f32<T>(0.0f);
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r, m = m0 + tx;
        if (c < C && m < Mp) out[(int64_t)c * ld_out + m] = tile[tx][r];
    }
}

// Bias gradients from dY^T, in a fixed order: workgroup (x, r) sums in[r][m] over its `per` chunks of 1024 * V columns
// (V = 16 / sizeof(T)) and stores the sum at out[x * slab_stride + r] -- a split-K slab of the bias segment, summed in
// ascending x by reduce_slabs_kernel like every other slab.  (Until the slabs carried them, each workgroup added its
// partial with an fp32 atomic: above one chunk the last bits depended on the arrival order.)  Every lane issues four
// independent 16-byte loads per chunk.
template <typename T>
__global__ __launch_bounds__(256) void rowsum_kernel(int Mp, int per, const T* __restrict__ in, int64_t ld_in, float* __restrict__ out,
                                                     int64_t slab_stride) {
    constexpr int V = 16 / sizeof(T);
    __shared__ float red[4];
    const T* row = in + (int64_t)blockIdx.y * ld_in;
    float s = 0.0f;
    for (int c = 0; c < per; ++c) {
        const int base = (blockIdx.x * per + c) * (256 * 4 * V);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int m = base + (u * 256 + threadIdx.x) * V;
            if (m < Mp) {   // Mp is a multiple of V and the pad columns are zero
                const u32x4 raw = *reinterpret_cast<const u32x4*>(row + m);
                const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
                for (int k = 0; k < V; ++k) s += to_f32<T>(e[k]);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[(int64_t)blockIdx.x * slab_stride + blockIdx.y] = red[0] + red[1] + red[2] + red[3];
}

// Auxiliary head loss: L = coef * mean_b mean_j (y[b][j] - t[b][j])^2 with t = priv[idx[b]][off + j].  Writes
// dL/dy in operand precision, row-major (dY, leading dimension ld) and transposed (dYT [No16][Mp]) for the generic backward,
// zero in the contraction padding rows B..Bp, and adds the (unweighted) minibatch MSE to opt[HGYM_OPT_AUX_SUM].
template <typename T>
__global__ __launch_bounds__(256) void aux_mse_kernel(int B, int Bp, int No, const float* __restrict__ y, const float* __restrict__ priv,
                                                      int64_t ldp, int off, const int64_t* __restrict__ idx, float coef,
                                                      T* __restrict__ dY, int64_t ld, T* __restrict__ dYT, int64_t ldt,
                                                      double* __restrict__ opt) {
    __shared__ float red[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float se = 0.0f;
    if (i < B) {
        const float* t = priv + idx[i] * ldp + off;
        const float g = 2.0f * coef / ((float)B * (float)No);
        for (int j = 0; j < No; ++j) {
            const float d = y[(int64_t)i * No + j] - t[j];
            se += d * d;
            const T gv = from_f32<T>(g * d);
            dY[(int64_t)i * ld + j] = gv;
            dYT[(int64_t)j * ldt + i] = gv;
        }
    } else if (i < Bp) {
        for (int j = 0; j < No; ++j) dYT[(int64_t)j * ldt + i] = from_f32<T>(0.0f);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) se += __shfl_down(se, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = se;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&opt[HGYM_OPT_AUX_SUM], (double)(red[0] + red[1] + red[2] + red[3]) / ((double)B * (double)No));
}

// PPO.act epilogue (actor_critic.py:111-120): a = mu + sigma*z, logp = sum log N(a; mu, sigma); sigma = std.
__global__ __launch_bounds__(256) void act_sample_kernel(int M, int A, const float* __restrict__ mu, const float* __restrict__ std_,
                                                         const float* __restrict__ z, uint64_t seed, const int64_t* __restrict__ step,
                                                         float* __restrict__ actions, float* __restrict__ sigma, float* __restrict__ logp) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    RngKey rk = {(uint32_t)seed, (uint32_t)(seed >> 32), 0u, 0u};
    if (!z) {
        const int64_t s = step ? step[0] : 0;
        rk.s0 = (uint32_t)s;
        rk.s1 = (uint32_t)(s >> 32);
    }
    float lp = 0.0f;
    float zn[16];
    if (!z) normals_block<4>(rk, (uint32_t)m, SLOT_POLICY, zn);
#pragma unroll
    for (int j = 0; j < 16; ++j) {      // fully unrolled so zn[] stays in registers
        if (j >= A) break;
        const float mj = mu[(int64_t)m * A + j];
        const float sg = mj * 0.0f + std_[j];            // actor_critic.py:113 (propagates NaN like the reference)
        const float zz = z ? z[(int64_t)m * A + j] : zn[j];
        const float a = mj + sg * zz;
        actions[(int64_t)m * A + j] = a;
        sigma[(int64_t)m * A + j] = sg;
        const float d = a - mj;
        lp += -(d * d) / (2.0f * sg * sg) - logf(sg) - 0.9189385332046727f;
    }
    logp[m] = lp;
}

// ppo_loss_kernel: hgym_loss.hpp (its instantiations with the mirror loss live in hgym_loss_mirror.hip)

// opt_state: the HGYM_OPT_* slots of include/hgym.h.
// grads_bmu / grads_bv (fused path only): gradients of the two head biases = column sums of the head gradients.
__global__ __launch_bounds__(512) void ppo_scalars_kernel(const ScalArgs a) { ppo_scalars_block(a, threadIdx.x, blockDim.x); }

// gradient finalise: sum the split-K slabs of every weight matrix and bias vector into the flat gradient vector
struct Segment {
    int64_t off;     // offset in the flat parameter vector
    int rows, cols;  // N, K  (bias / std: rows = count, cols = 1, no shadow)
    int splits;      // slabs to sum (0: gradient already final in `grads`)
    void* Wp;        // operand-precision shadow [N16][ldw] or null
    int64_t ldw;
    void* WTp;       // operand-precision transposed shadow [K16][ldwt] or null
    int64_t ldwt;
    void* Wf;        // fused path: forward fragments [NB][KB][64][8] or null
    void* WTf;       // fused path: backward fragments [K/16][NBB][64][8]
    int KB, NBB;
    float* sigma;    // the std segment in HGYM_STD_LOG: the derived sigma block, rewritten wherever the parameter is; null otherwise
};
struct SegTable {
    int n;
    Segment s[2 * HGYM_MAX_LAYERS * 2 + 1];
};
// Observation normalisation (HgymNet.norm, hgym_norm.hip): per segment of a table, the per-column scale its operand copies carry -- T(w * cs[c])
// instead of T(w) -- for the first-layer weight segments, null for every other.  An argument of adam_norm_kernel / sync_shadow_norm_kernel only: a
// net without normalisation launches adam_kernel / sync_shadow_kernel with the arguments they always had.
struct NormCols {
    const float* cs[2 * HGYM_MAX_LAYERS * 2 + 1];
};

// Also accumulates the squared norm of the finished gradient into opt[HGYM_OPT_GRAD_SQNORM] (zeroed by ppo_scalars_kernel earlier in the same
// hgym_ppo_grad): with one rank that IS the norm clip_grad_norm_ needs, and hgym_ppo_apply skips its own pass over the
// gradient.  (Segments whose gradient is already final -- splits == 0 -- are only read.)
// The norm stays on fp64 atomics in arrival order (1 632 workgroups, one non-returning atomicAdd each) -- made order-INDEPENDENT by rounding every
// partial to a common quantum first (below): exact additions commute.  Round 6 first built the order-fixed forms -- per-workgroup partials + last
// arriver with a release fence per workgroup: 65 us instead of 11 (every fence writes the XCD's L2 back while the others fill it with gradient
// lines); write-through partials + acknowledged store + returning counter atomic, on one and on two levels: 26-29 us (three to six dependent
// memory-side round trips at the tail of an 11 us kernel) -- and dropped them (profiles/r06_update_graph_and_norm_order.txt).  With several ranks
// the norm is sqnorm_prologue_kernel's, which is order-fixed (256 workgroups, one launch).
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const SegTable tab, int64_t P, const float* __restrict__ slabs,
                                                           float* __restrict__ grads, double* __restrict__ opt) {
    __shared__ double red[4];
    const Segment& sg = tab.s[blockIdx.y];
    const int64_t n = (int64_t)sg.rows * sg.cols;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double sq = 0.0;
    if (sg.splits == 0) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
            const float g = grads[sg.off + i];
            sq += (double)g * (double)g;
        }
    } else {
        // 16-byte body between a scalar head and tail: a segment need not start on a 16-byte boundary of the flat vector (the
        // critic's one-element head bias puts every segment of the auxiliary net at offset = 1 mod 4)
        const bool vec = (P & 3) == 0 && (((uintptr_t)grads | (uintptr_t)slabs) & 15) == 0;      // P = slab stride
        const int64_t head = vec ? ((4 - (sg.off & 3)) & 3) < n ? ((4 - (sg.off & 3)) & 3) : n : n;
        const int64_t n4 = (n - head) >> 2, tail0 = head + 4 * n4;
        const int64_t base = sg.off + head;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (sg.splits == 8) {      // the usual split count: all eight loads in flight, then the same ascending sum
                float4 v[8];
#pragma unroll
                for (int z = 0; z < 8; ++z) v[z] = *reinterpret_cast<const float4*>(slabs + (int64_t)z * P + base + 4 * i);
#pragma unroll
                for (int z = 0; z < 8; ++z) { acc.x += v[z].x; acc.y += v[z].y; acc.z += v[z].z; acc.w += v[z].w; }
            } else {
                for (int z = 0; z < sg.splits; ++z) {
                    const float4 v = *reinterpret_cast<const float4*>(slabs + (int64_t)z * P + base + 4 * i);
                    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
                }
            }
            *reinterpret_cast<float4*>(grads + base + 4 * i) = acc;
            sq += (double)acc.x * (double)acc.x + (double)acc.y * (double)acc.y + (double)acc.z * (double)acc.z + (double)acc.w * (double)acc.w;
        }
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < head + (n - tail0); i += stride) {
            const int64_t e = i < head ? i : tail0 + (i - head);
            float s = 0.0f;
            for (int z = 0; z < sg.splits; ++z) s += slabs[(int64_t)z * P + sg.off + e];
            grads[sg.off + e] = s;
            sq += (double)s * (double)s;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_down(sq, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        // Pre-rounded to a common quantum (2^-46): every partial, and therefore every intermediate value of opt[GRAD_SQNORM], is an integer multiple of
        // it, so while the total stays below 2^53 quanta = 128 (a gradient norm of 11.3, eleven times the clip threshold) the fp64 additions
        // are EXACT -- and exact additions commute: the atomics may arrive in any order, the sum has the same bits.  (Above 128 the additions
        // round again and the last bits depend on the order, as they always did; the step is then clipped by more than 11x and sees `total`
        // as a float.)  Cost of the rounding: at most 1 632 x 2^-47 = 1.2e-11 absolute on the squared norm.
        double t = red[0] + red[1] + red[2] + red[3];
        t = __builtin_rint(t * 0x1p46) * 0x1p-46;
        if (t != 0.0) atomicAdd(&opt[HGYM_OPT_GRAD_SQNORM], t);
    }
}

// (inv_w: 1 / world_size -- with several ranks the gradient vector holds the all-reduced SUM and the mean is formed in sqnorm_prologue_kernel and in
// adam_kernel: an fp32 product, what `grad.mul_(1 / world)` would have stored; 1.0f for one rank, which is exact.)

// ppo.py:140-148 (adaptive-KL learning rate: adapt_lr, hgym_fused.hpp) + Adam step counter + the squared norm Adam will clip with: `sq` when
// this call determined it itself (sqnorm_prologue_kernel), 0 when a norm pass follows, untouched when the gradient call left it (have_sq < 0)
__device__ __forceinline__ void apply_prologue(const HgymPPOConfig& p, const float* __restrict__ kl_slot, float inv_w, double* __restrict__ opt,
                                               int have_sq, double sq) {
    if (p.world_size > 1) opt[HGYM_OPT_KL_LAST] = (double)(kl_slot[0] * inv_w);     // mean over ranks of the minibatch KL: same LR branch everywhere
    if (PROLOGUE_PENDING(opt)) {     // the gradient call already took this step's prologue (marker: ppo_scalars_block) and the
        if (have_sq >= 0) opt[HGYM_OPT_GRAD_SQNORM] = have_sq ? sq : 0.0;                // caller applies with another configuration: not a second time
        return;
    }
    if (p.adaptive_lr) opt[HGYM_OPT_LR] = adapt_lr(opt[HGYM_OPT_LR], (float)opt[HGYM_OPT_KL_LAST], p.desired_kl, p.lr_min, p.lr_max);      // (KL_LAST as the caller left it: rounded)
    const double t = opt[HGYM_OPT_STEP] + 1.0;
    opt[HGYM_OPT_STEP] = t;
    // Adam's bias corrections, once per step instead of two double-precision pow() per thread of adam_kernel (1.1 M threads): the
    // same double arithmetic, rounded to the floats the update uses
    const bool cached = opt[HGYM_OPT_PROLOGUE_STEP] == t;             // ppo_scalars_block left beta^t of this step (same pow(), same arguments): kernel 8.1 -> 4.8 us
    const double bc1 = 1.0 - (cached ? opt[HGYM_OPT_BETA1_POW] : pow((double)p.beta1, t)), bc2 = 1.0 - (cached ? opt[HGYM_OPT_BETA2_POW] : pow((double)p.beta2, t));
    opt[HGYM_OPT_STEP_SIZE] = (double)(float)(opt[HGYM_OPT_LR] / bc1);      // step size
    opt[HGYM_OPT_SQRT_BC2] = (double)(float)sqrt(bc2);
    opt[HGYM_OPT_PROLOGUE_STEP] = t;                              // marker: this step's prologue is done (adam_kernel clears it)
    if (have_sq >= 0) opt[HGYM_OPT_GRAD_SQNORM] = have_sq ? sq : 0.0;
}
__global__ void apply_prologue_kernel(const HgymPPOConfig p, const float* __restrict__ kl_slot, float inv_w, double* __restrict__ opt) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    // (a norm pass follows this launch only when the caller could not reuse the gradient call's: several ranks / foreign gradients)
    apply_prologue(p, kl_slot, inv_w, opt, (p.world_size > 1 || !p.grad_norm_ready) ? 0 : -1, 0.0);
}

// The two launches hgym_ppo_apply used to start with when the norm of the gradient call cannot be reused (several ranks: the norm is of the
// rank MEAN; foreign gradients) -- the prologue and the squared-norm pass -- as one: every workgroup leaves its fp64 partial sum, the last one
// to arrive adds the SQN_BLOCKS partials in a fixed order (no atomics on the sum: the same bits on every rank and in every run) and takes the
// prologue with the total.  part[SQN_BLOCKS] is the arrival counter (an unsigned int, zero between launches: the last workgroup resets it).
__global__ __launch_bounds__(256) void sqnorm_prologue_kernel(int64_t P, const float* __restrict__ g, float inv_w, const HgymPPOConfig p,
                                                              const float* __restrict__ kl_slot, double* __restrict__ opt,
                                                              double* __restrict__ part) {
    __shared__ double red[4];
    __shared__ unsigned int s_last;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * inv_w;
        s += (double)gi * (double)gi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    unsigned int* counter = reinterpret_cast<unsigned int*>(part + SQN_BLOCKS);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
        __threadfence();
        s_last = atomicAdd(counter, 1u) == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    double v = threadIdx.x < gridDim.x ? reinterpret_cast<const volatile double*>(part)[threadIdx.x] : 0.0;      // (behind the fence: the peers' partials)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        *counter = 0u;
        apply_prologue(p, kl_slot, inv_w, opt, 1, red[0] + red[1] + red[2] + red[3]);
    }
}

// HGYM_STD_LOG: sigma from its parameter log sigma -- the ONE place that forms it (adam_kernel behind a step, sync_shadow_kernel behind a
// load; everything that reads sigma reads the block they fill).  expf: 1 ulp as HIP documents it; exp(0) = 1 exactly.
__device__ __forceinline__ float sigma_of(float log_sigma) { return expf(log_sigma); }

// writes one master weight into every compute-precision operand copy of its layer
template <typename T>
__device__ __forceinline__ void write_shadows(const Segment& sg, int r, int c, float w) {
    if (sg.Wp) {
        ((T*)sg.Wp)[(int64_t)r * sg.ldw + c] = from_f32<T>(w);
        if (sg.WTp) ((T*)sg.WTp)[(int64_t)c * sg.ldwt + r] = from_f32<T>(w);
    }
    if (sg.Wf) {   // r = n (output feature), c = k (input feature); see hgym_fused.hpp for the fragment order
        ((T*)sg.Wf)[((((int64_t)(r >> 4) * sg.KB + (c >> 5)) * 64) + ((c & 31) >> 3) * 16 + (r & 15)) * 8 + (c & 7)] = from_f32<T>(w);
        ((T*)sg.WTf)[((((int64_t)(c >> 4) * sg.NBB + (r >> 5)) * 64) + ((r & 31) >> 3) * 16 + (c & 15)) * 8 + (r & 7)] = from_f32<T>(w);
    }
}

// One body for adam_kernel and its twin for a normalised net.  colscale: null, or -- a first-layer weight segment of a normalised net (HgymNet.norm,
// hgym_norm.hip) -- the per-column scale its operand copies carry, T(w * colscale[c]) instead of T(w).  adam_kernel passes a literal null, which
// folds: it keeps the arguments and the code it had before the feature existed.
template <typename T>
__device__ __forceinline__ void adam_body(const Segment& sg, const HgymPPOConfig& p, float* params, float* grads, float* m_, float* v_, float inv_w,
                                          double* opt, const float* colscale) {
    const int64_t n = (int64_t)sg.rows * sg.cols;
    // nn.utils.clip_grad_norm_: coef = max_norm / (total_norm + 1e-6), clamped to 1 (fp32 tensor arithmetic)
    const float total = (float)sqrt(opt[HGYM_OPT_GRAD_SQNORM]);
    float coef = p.max_grad_norm / (total + 1e-6f);
    coef = fminf(coef, 1.0f);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        opt[HGYM_OPT_GRAD_NORM] = (double)total;
        opt[HGYM_OPT_PROLOGUE_STEP] = -1.0;       // the step whose prologue was pending is being applied (nobody reads the marker in this launch)
    }
    const float step_size = (float)opt[HGYM_OPT_STEP_SIZE], sqrt_bc2 = (float)opt[HGYM_OPT_SQRT_BC2];      // apply_prologue_kernel: lr / (1 - beta1^t), sqrt(1 - beta2^t)
    auto adam1 = [&](int64_t q) -> float {            // one parameter: clip, moments, step; returns the new weight
        const float g = (grads[q] * inv_w) * coef;
        grads[q] = g;
        const float m = m_[q] * p.beta1 + (1.0f - p.beta1) * g;
        const float v = v_[q] * p.beta2 + (1.0f - p.beta2) * (g * g);
        m_[q] = m;
        v_[q] = v;
        const float denom = sqrtf(v) / sqrt_bc2 + p.adam_eps;
        const float w = params[q] + (-step_size * m) / denom;
        params[q] = w;
        return w;
    };
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float w = adam1(sg.off + i);
        if (sg.Wp || sg.Wf) {
            const int r = (int)(i / sg.cols), c = (int)(i - (int64_t)r * sg.cols);
            write_shadows<T>(sg, r, c, colscale ? w * colscale[c] : w);
        } else if (sg.sigma) {
            sg.sigma[i] = sigma_of(w);      // same launch: a captured update keeps the block current without a node of its own
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void adam_kernel(const SegTable tab, const HgymPPOConfig p, float* __restrict__ params,
                                                   float* __restrict__ grads, float* __restrict__ m_, float* __restrict__ v_,
                                                   float inv_w, double* __restrict__ opt) {
    adam_body<T>(tab.s[blockIdx.y], p, params, grads, m_, v_, inv_w, opt, nullptr);
}
template <typename T>
__global__ __launch_bounds__(256) void adam_norm_kernel(const SegTable tab, const HgymPPOConfig p, float* __restrict__ params,
                                                        float* __restrict__ grads, float* __restrict__ m_, float* __restrict__ v_,
                                                        float inv_w, double* __restrict__ opt, const NormCols nc) {
    adam_body<T>(tab.s[blockIdx.y], p, params, grads, m_, v_, inv_w, opt, nc.cs[blockIdx.y]);
}

template <typename T>
__device__ __forceinline__ void sync_shadow_body(const Segment& sg, const float* params, const float* colscale) {
    if (sg.sigma)       // (ahead of the early return: the std segment has no operand copy, but in log mode it has this one)
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)sg.rows * sg.cols; i += (int64_t)gridDim.x * blockDim.x)
            sg.sigma[i] = sigma_of(params[sg.off + i]);
    if (!sg.Wp && !sg.Wf) return;
    const int64_t n = (int64_t)sg.rows * sg.cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / sg.cols), c = (int)(i - (int64_t)r * sg.cols);
        write_shadows<T>(sg, r, c, colscale ? params[sg.off + i] * colscale[c] : params[sg.off + i]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void sync_shadow_kernel(const SegTable tab, const float* __restrict__ params) {
    sync_shadow_body<T>(tab.s[blockIdx.y], params, nullptr);
}
template <typename T>
__global__ __launch_bounds__(256) void sync_shadow_norm_kernel(const SegTable tab, const float* __restrict__ params, const NormCols nc) {
    sync_shadow_body<T>(tab.s[blockIdx.y], params, nc.cs[blockIdx.y]);
}

// ------------------------------------------------------------------------------------------------ GEMM dispatch
template <typename T, int BM, int BN, int WMs, int WNs>
static void launch_cfg(const GemmArgs& g, int splits, hipStream_t s) {
    constexpr int F = ((BM / 16) + (BN / 16)) * KSTAGE;
    constexpr size_t lds = (size_t)2 * F * 1024;
    // > 64 KiB of LDS needs the opt-in, per device (a failure surfaces as the launch error the caller checks)
    (void)ensure_dynamic_lds(reinterpret_cast<const void*>(&gemm_nt_kernel<T, BM, BN, WMs, WNs>), lds, "gemm_nt_kernel");
    dim3 grid(ceil_div(g.N, BN), ceil_div(g.M, BM), splits);
    hipLaunchKernelGGL((gemm_nt_kernel<T, BM, BN, WMs, WNs>), grid, dim3(WMs * WNs * 64), lds, s, g);
}

template <typename T>
int32_t launch_gemm(const GemmArgs& g0, int splits, hipStream_t s) {
    GemmArgs g = g0;
    constexpr int SE = stage_elems<T>();
    HG_REQUIRE(g.K % SE == 0 && g.K > 0, HGYM_E_SHAPE, "gemm K=%d not a multiple of %d", g.K, SE);
    HG_REQUIRE(g.lda * (int64_t)sizeof(T) % 16 == 0 && g.ldb * (int64_t)sizeof(T) % 16 == 0, HGYM_E_SHAPE, "gemm operand rows must be 16-byte aligned");
    if (splits < 1) splits = 1;
    int stages = g.K / SE;
    if (splits > stages) splits = stages;
    const int per = ceil_div(stages, splits);
    splits = ceil_div(stages, per);
    g.k_chunk = per * SE;
    prof_begin(HGYM_PROF_GEMM, s);
    // (the tile choice is restated in tests/layer_path_common.py: tile -- keep the two in step)
    const int64_t t128 = (int64_t)ceil_div(g.M, 128) * ceil_div(g.N, 128) * splits;
    if (g.N <= 16) launch_cfg<T, 128, 16, 4, 1>(g, splits, s);
    else if (g.M <= 16) launch_cfg<T, 16, 128, 1, 4>(g, splits, s);
    else if (t128 >= 192) launch_cfg<T, 128, 128, 2, 2>(g, splits, s);
    else launch_cfg<T, 64, 64, 2, 2>(g, splits, s);
    prof_end(HGYM_PROF_GEMM, s, 2.0 * (double)g.M * (double)g.N * (double)g.K);   // padded K: the flops the MFMAs execute
    HG_CHECK_LAUNCH("gemm_nt_kernel");
    return splits;
}

// ------------------------------------------------------------------------------------------------ orchestration
// input rows and output of one net in a launch (arrays of three are indexed by net id)
struct NetIO {
    const float* x;
    int64_t ldx;
    float* out;
    int64_t ldo;
};

// bf16 shadow rows of net `which`'s input on the fused layout (hgym_net_shadow_ld): the first layer's padded width
static int64_t shadow_ld(const WsLayout& w, int which) { return (int64_t)w.net[which].layer[0].KBf * 32; }

static int32_t check_shadow(const WsLayout& w, const HgymObsShadow* sh) {
    if (!sh) return HGYM_OK;
    HG_REQUIRE((!sh->obs || (sh->ld_obs >= shadow_ld(w, 0) && sh->ld_obs % 8 == 0 && ((uintptr_t)sh->obs & 15) == 0)) &&
                   (!sh->priv || (sh->ld_priv >= shadow_ld(w, 1) && sh->ld_priv % 8 == 0 && ((uintptr_t)sh->priv & 15) == 0)),
               HGYM_E_SHAPE, "observation shadow: leading dimensions %lld / %lld (need >= %lld / %lld, multiples of 8, 16-byte aligned rows)",
               (long long)sh->ld_obs, (long long)sh->ld_priv, (long long)shadow_ld(w, 0), (long long)shadow_ld(w, 1));
    return HGYM_OK;
}

// dynamic LDS of one mlp_fwd_kernel launch with BM-row tiles over a.net[a.net0 .. + nets)
static size_t fwd_lds(const FwdArgs& a, int nets, int BM) {
    size_t lds = 0;
    for (int i = 0; i < nets; ++i) lds = std::max(lds, (size_t)fwd_lds_bytes(a.net[a.net0 + i], BM));
    return lds;
}

// Where the kernels read sigma: the head of the parameter vector (HGYM_STD_SCALAR) or the derived block (HGYM_STD_LOG).  Every site that
// hands sigma to a kernel goes through here.
static const float* sigma_src(const WsLayout& w, const HgymNet& net) {
    return w.sigma >= 0 ? reinterpret_cast<const float*>((const char*)net.workspace + w.sigma) : net.params;
}

// What both paths share: the workspace, the segment table of the slab reduction / Adam / the shadow refresh, and those two launches.
struct NetBase {
    const HgymNetConfig& cfg;
    const HgymNet& net;
    const WsLayout& w;
    hipStream_t s;
    char* ws;

    NormLayout nl;           // observation normalisation (net.norm set): the block's layout, else zero
    template <typename U> U* at(int64_t off) const { return reinterpret_cast<U*>(ws + off); }
    template <typename U> U* norm_at(int64_t off) const { return reinterpret_cast<U*>((char*)net.norm + off); }
    // The bias the kernels add behind layer l of net `which`: the parameter, or -- first layer of a normalised net -- the effective bias
    // b - (W o s) m that norm_fold_bias keeps in the block.  Every site that hands a bias to a kernel goes through here.
    const float* bias_in(int which, int l) const {
        return (l == 0 && net.norm) ? norm_at<float>(nl.eb[which]) : net.params + w.net[which].layer[l].b_off;
    }
    const float* sigma_in() const { return sigma_src(w, net); }
    // ScalArgs::sigma: the chain-rule factor of the std gradient (log mode), null where the gradient is sigma's own
    const float* grad_sigma() const { return w.sigma >= 0 ? sigma_in() : nullptr; }

    // split-K slabs of a weight gradient on the layer-by-layer path, for a minibatch whose contraction padding is Mp
    // (restated in tests/layer_path_common.py: split_count -- keep the two in step)
    int split_count(const LayerLayout& y, int Mp) const {
        // enough workgroups to fill 256 CUs: tiles(N x K) x splits ~ 512
        const int tiles = ceil_div(y.N, y.N <= 16 ? 16 : 128) * ceil_div(y.K, 128);
        int sp = ceil_div(512, tiles);
        if (sp > w.splits) sp = w.splits;
        const int stages = Mp / w.SE;
        if (sp > stages) sp = stages;
        if (sp < 1) sp = 1;
        const int per = ceil_div(stages, sp);
        return ceil_div(stages, per);
    }

    // rowsum_kernel's workgroups per bias row (= its slabs) for a minibatch of contraction padding Mp, and the chunks each one sums
    // (restated in tests/layer_path_common.py: rowsum_splits)
    int rowsum_splits(int Mp, int* per_out = nullptr) const {
        const int chunks = ceil_div(Mp, 1024 * 16 / w.es);
        const int per = ceil_div(chunks, std::min(chunks, w.splits));
        if (per_out) *per_out = per;
        return ceil_div(chunks, per);
    }

    // Mp > 0: with the slab counts of a gradient over a minibatch of contraction padding Mp; Mp = 0: without (Adam, shadow refresh)
    SegTable segments(int Mp) const {
        SegTable t;
        memset(&t, 0, sizeof(t));
        Segment& sd = t.s[t.n++];
        sd.off = 0;
        sd.rows = cfg.num_actions;
        sd.cols = 1;
        if (w.sigma >= 0) sd.sigma = at<float>(w.sigma);
        for (int which = 0; which < w.nnets; ++which) {
            const NetLayout& n = w.net[which];
            for (int l = 0; l < n.L; ++l) {
                const LayerLayout& y = n.layer[l];
                Segment& a = t.s[t.n++];
                a.off = y.w_off;
                a.rows = y.N;
                a.cols = y.K;
                if (n.fused) {
                    a.splits = Mp ? w.dw_splits : 0;
                    a.Wf = ws + y.Wf;
                    a.WTf = ws + y.WTf;
                    a.KB = y.KBf;
                    a.NBB = y.NBBf;
                } else {
                    a.splits = Mp ? split_count(y, Mp) : 0;
                    a.Wp = ws + y.Wp;
                    a.ldw = y.Kp;
                    a.WTp = ws + y.WTp;
                    a.ldwt = y.Ncp;
                }
                Segment& b = t.s[t.n++];
                b.off = y.b_off;
                b.rows = y.N;
                b.cols = 1;
                // bias gradients that come from the slabs: on the fused layout the hidden layers' (the dW kernel's column sums of dZ;
                // the actor / critic head biases are written by ppo_scalars_kernel, the auxiliary head's is a column sum like the others)
                if (n.fused && Mp && (l < n.L - 1 || which == 2)) b.splits = w.dw_splits;
                if (!n.fused && Mp) b.splits = rowsum_splits(Mp);     // every bias of a layer-by-layer net: rowsum_kernel's slabs
            }
        }
        return t;
    }

    // The scale pointers that go with segments(): the table's order -- std, then weight | bias of every layer of every net
    NormCols norm_cols() const {
        NormCols nc;
        memset(&nc, 0, sizeof(nc));
        int i = 1;
        for (int which = 0; which < w.nnets; ++which)
            for (int l = 0; l < w.net[which].L; ++l, i += 2)
                if (l == 0 && net.norm) nc.cs[i] = norm_at<float>(nl.sf[which == 1 ? 1 : 0]);
        return nc;
    }

    // prologue_done: the gradient call has already taken the learning-rate decision and Adam's step scalars (FusedPath::prologue_in_grad)
    template <typename T>
    int32_t apply(const HgymPPOConfig& ppo, bool prologue_done) {
        HG_REQUIRE(!net.norm || !ppo.grad_norm_ready, HGYM_E_BADARG,
                   "HgymPPOConfig.grad_norm_ready = 1 with HgymNet.norm set: hgym_net_norm_unfold_grad changes the gradient behind hgym_ppo_grad");
        prof_begin(HGYM_PROF_APPLY, s);
        const float inv_w = ppo.world_size > 1 ? (float)(1.0 / (double)ppo.world_size) : 1.0f;
        if (ppo.world_size > 1 || !ppo.grad_norm_ready)        // else: reduce_slabs_kernel left the squared norm in opt[HGYM_OPT_GRAD_SQNORM]
            hipLaunchKernelGGL(sqnorm_prologue_kernel, dim3(SQN_BLOCKS), dim3(256), 0, s, w.P, net.grads, inv_w, ppo, net.grads + w.P, net.opt_state,
                               at<double>(w.sqn));
        else if (!prologue_done)
            hipLaunchKernelGGL(apply_prologue_kernel, dim3(1), dim3(64), 0, s, ppo, net.grads + w.P, inv_w, net.opt_state);
        const SegTable tab = segments(0);
        // 256 workgroups per segment: the two first-layer matrices hold 57 % of the parameters, and 64 workgroups (a quarter of
        // the CUs) walked them in 22 dependent load -> store rounds per lane (30.7 us; 18.1 us with 256, 20.8 us with 512)
        if (net.norm)
            hipLaunchKernelGGL((adam_norm_kernel<T>), dim3(256, tab.n), dim3(256), 0, s, tab, ppo, net.params, net.grads, net.adam_m, net.adam_v,
                               inv_w, net.opt_state, norm_cols());
        else
            hipLaunchKernelGGL((adam_kernel<T>), dim3(256, tab.n), dim3(256), 0, s, tab, ppo, net.params, net.grads, net.adam_m, net.adam_v,
                               inv_w, net.opt_state);
        {   // HBM bytes the launches above move: adam_body reads and rewrites gradient, both moments and the master weight (32 B per
            // parameter) and stores every weight's two operand copies (2 sizeof(T) B per weight; biases and std have none -- in log mode
            // std has its derived sigma, 4 B); sqnorm_prologue_kernel, where it runs, reads the gradient once more (4 B per parameter)
            double bytes = 32.0 * (double)w.P;
            for (int i = 0; i < tab.n; ++i) {
                const double n = (double)tab.s[i].rows * tab.s[i].cols;
                if (tab.s[i].Wp || tab.s[i].Wf) bytes += 2.0 * sizeof(T) * n;
                else if (tab.s[i].sigma) bytes += 4.0 * n;
            }
            if (ppo.world_size > 1 || !ppo.grad_norm_ready) bytes += 4.0 * (double)w.P;
            prof_end(HGYM_PROF_APPLY, s, bytes);
        }
        HG_CHECK_LAUNCH("adam_kernel");
        return net.norm ? norm_fold_bias(&cfg, &net, s) : HGYM_OK;      // the first-layer weights moved: their effective biases follow
    }

    template <typename T>
    int32_t sync_shadow() {
        const SegTable tab = segments(0);
        if (net.norm) hipLaunchKernelGGL((sync_shadow_norm_kernel<T>), dim3(64, tab.n), dim3(256), 0, s, tab, net.params, norm_cols());
        else hipLaunchKernelGGL((sync_shadow_kernel<T>), dim3(64, tab.n), dim3(256), 0, s, tab, net.params);
        HG_CHECK_LAUNCH("sync_shadow_kernel");
        return net.norm ? norm_fold_bias(&cfg, &net, s) : HGYM_OK;
    }

    // hgym_bc_grad, both paths.  bc_zero_grads: the whole gradient vector and the KL slot to +0.0 ahead of the step's launches -- what a
    // cloning step does not train (std, critic, auxiliary head) must leave Adam with nothing to apply.  bc_reduce_actor: reduce_range over
    // the actor's segments alone (and, through them, the squared norm: every other entry is zero).
    int32_t bc_zero_grads() {
        return zero_f32_async(net.grads, w.P + 1, s);      // a launch, not a memset node: the step also runs inside captured updates (hgym_fill.hip)
    }
    int32_t bc_reduce_actor(int Mp) { return reduce_range(w.net[0].layer[0].w_off, w.net[1].layer[0].w_off, Mp); }
    // hgym_vf_grad / hgym_bc_vf_grad: the critic's segments alone; the actor's and the critic's in one pass
    int32_t vf_reduce_critic(int Mp) { return reduce_range(w.net[1].layer[0].w_off, w.aux_p0, Mp); }
    int32_t bc_vf_reduce(int Mp) { return reduce_range(w.net[0].layer[0].w_off, w.aux_p0, Mp); }

    // slab reduction of the segments whose parameters lie in [lo, hi) of the flat vector (Mp: an auxiliary head on the layer-by-layer
    // path took its slab counts from the minibatch's contraction padding)
    int32_t reduce_range(int64_t lo, int64_t hi, int Mp) {
        const SegTable all = segments(Mp);
        SegTable tab;
        memset(&tab, 0, sizeof(tab));
        int64_t elems = 0;
        for (int i = 0; i < all.n; ++i)
            if (all.s[i].off >= lo && all.s[i].off < hi) {
                tab.s[tab.n++] = all.s[i];
                elems += (int64_t)all.s[i].rows * all.s[i].cols;
            }
        if (tab.n == 0) return HGYM_OK;
        prof_begin(HGYM_PROF_REDUCE, s);
        hipLaunchKernelGGL(reduce_slabs_kernel, dim3(RSN_X, tab.n), dim3(256), 0, s, tab, w.Ps, at<float>(w.slabs), net.grads, net.opt_state);
        prof_end(HGYM_PROF_REDUCE, s, (double)elems * 4.0 * (w.dw_splits + 1));
        HG_CHECK_LAUNCH("reduce_slabs_kernel");
        return HGYM_OK;
    }

    // Observation normalisation, after the statistics moved: the operand copies of the first-layer weights (the only ones that hold the
    // scale) and the effective biases.
    template <typename T>
    int32_t norm_refold() {
        const SegTable all = segments(0);
        const NormCols cols = norm_cols();
        SegTable tab;
        NormCols nc;
        memset(&tab, 0, sizeof(tab));
        memset(&nc, 0, sizeof(nc));
        for (int i = 0; i < all.n; ++i)
            if (cols.cs[i]) {
                nc.cs[tab.n] = cols.cs[i];
                tab.s[tab.n++] = all.s[i];
            }
        hipLaunchKernelGGL((sync_shadow_norm_kernel<T>), dim3(64, tab.n), dim3(256), 0, s, tab, net.params, nc);
        HG_CHECK_LAUNCH("sync_shadow_norm_kernel");
        return norm_fold_bias(&cfg, &net, s);
    }
};

// hgym_ppo_grad_smooth's pre-passes on either path, ahead of everything else of the call: the targets of the two terms under the current
// parameters, forward only (no gradient through a target).  Both read fp32 rows, as the mirror loss's pre-pass does.  The perturbation comes
// first of all: it reads opt_state[HGYM_OPT_STEP], which the loss-scalar workgroup of this very call may advance.
inline int smooth_ld(int num_obs) { return (num_obs + 3) / 4 * 4; }
template <class R>
static int32_t smooth_prepass(R& r, const HgymBatch& b, const HgymSmooth& sm) {
    const int B = b.B, A = r.cfg.num_actions;
    if (sm.spatial_coef > 0.0f) {
        const int ld = smooth_ld(r.cfg.num_obs);
        int32_t rc = launch_perturb_rows(B, r.cfg.num_obs, b.obs, r.cfg.num_obs, b.idx, sm.noise_std, sm.seed, r.net.opt_state, sm.rows, ld, r.s);
        if (rc) return rc;
        rc = r.forward(0, B, sm.rows, ld, nullptr, sm.target_near, A, false);
        if (rc) return rc;
    }
    if (sm.temporal_coef > 0.0f) {
        const int32_t rc = r.forward(0, B, b.obs, r.cfg.num_obs, sm.next_idx, sm.target_next, A, false);
        if (rc) return rc;
    }
    return HGYM_OK;
}
inline bool smooth_on(const HgymSmooth* sm) { return sm && (sm->temporal_coef > 0.0f || sm->spatial_coef > 0.0f); }

// The actor's head of one hgym_ppo_grad* call: what joins d mu beside the PPO term, resolved once (actor_head) for both runners.
//   sm (hgym_ppo_grad_smooth): the smoothness regulariser joins d mu; null or both coefficients 0: off, the launches of hgym_ppo_grad
//   hp (hgym_ppo_grad_smooth_mirror): head_partials, carried only when the mirror loss and the regulariser are both on
//   gd (hgym_ppo_grad_guide): the teacher's term joins d mu; never together with the mirror loss or sm
struct ActorHead {
    enum Kind { PLAIN, MIRROR, SMOOTH, MIRROR_SMOOTH, GUIDE } kind;      // (a pointer or a scale that the kind does not use stays null / 0)
    const HgymSmooth* sm;
    float* hp;
    const HgymGuide* gd;
    float m_g;               // 2 * mirror_coef / (B * A)
    float gT, gS;            // 2 * temporal_coef / (B * A), 2 * spatial_coef / (B * A)
    float inv2;              // the guide's 2 / (B * A)
    bool mirror() const { return kind == MIRROR || kind == MIRROR_SMOOTH; }
    bool smooth() const { return kind == SMOOTH || kind == MIRROR_SMOOTH; }
};

// The scales are fp32 kernel arguments: each is formed by the one expression, in the one operation order, it always had.
static ActorHead actor_head(const HgymPPOConfig& ppo, int B, int A, const HgymSmooth* sm, float* hp, const HgymGuide* gd) {
    const bool mirror = ppo.mirror_coef > 0.0f, smooth = smooth_on(sm);
    // (gd arrives only with both off: hgym_ppo_grad_guide refuses the mirror loss and hands over no HgymSmooth)
    const bool guide = gd && !mirror && !smooth;
    const ActorHead::Kind kind = mirror ? (smooth ? ActorHead::MIRROR_SMOOTH : ActorHead::MIRROR) : (smooth ? ActorHead::SMOOTH : (guide ? ActorHead::GUIDE : ActorHead::PLAIN));
    ActorHead h = {kind, smooth ? sm : nullptr, mirror && smooth ? hp : nullptr, guide ? gd : nullptr, 0.0f, 0.0f, 0.0f, 0.0f};
    if (mirror) h.m_g = 2.0f * ppo.mirror_coef / ((float)B * (float)A);
    if (smooth) {
        const float gs = 2.0f / ((float)B * (float)A);
        h.gT = gs * sm->temporal_coef;
        h.gS = gs * sm->spatial_coef;
    }
    if (guide) h.inv2 = 2.0f / ((float)B * (float)A);
    return h;
}

// The head's pre-passes on either path, ahead of everything else of the call: the smoothness regulariser's first (hgym_ppo_grad_smooth_mirror's order;
// alone, either is the only one), then the mirror loss's -- the raw mu of the partner rows under the current parameters, forward only (no gradient
// through the target).  On the fused path it gathers the fp32 rows, not their bf16 shadow: the forward tiles that gather by index from a shadow
// exist in the update kernels only, and the shadow is bf16(fp32 row) exactly -- the same bits reach the first layer either way.
template <class R>
static int32_t head_prepass(R& r, const HgymBatch& b, const ActorHead& h) {
    if (h.smooth()) {
        const int32_t rc = smooth_prepass(r, b, *h.sm);
        if (rc) return rc;
    }
    if (h.mirror()) return r.forward(0, b.B, b.obs, r.cfg.num_obs, b.pair_idx, b.mirror_target, r.cfg.num_actions, false);
    return HGYM_OK;
}

// Behind the head's launch on either path: the sums of the head's own squared errors from the n partial rows it left (n: the fused path's tiles,
// the layer-by-layer path's loss blocks).  The mirror loss alone has none: its sum rides with the loss scalars (ScalArgs::mirror_sums).
static int32_t head_sums(const ActorHead& h, int n, int B, int A, const float* partials, hipStream_t s) {
    switch (h.kind) {
    case ActorHead::MIRROR_SMOOTH: return launch_head_sums(n, B, A, h.hp, h.sm->next_weight, h.sm->sums, s);
    case ActorHead::SMOOTH: return launch_smooth_sums(n, B, A, partials, h.sm->next_weight, h.sm->sums, s);
    case ActorHead::GUIDE: return launch_guide_sums(n, B, A, partials, h.gd->sums, s);
    default: return HGYM_OK;
    }
}

// The layer-by-layer path: every dense product through gemm_nt_kernel in the operand precision T, plus the packs, transposes and
// row sums around it.
template <typename T>
struct GemmPath : NetBase {
    int32_t forward(int which, int M, const float* x, int64_t ldx, const int64_t* idx, float* y_out, int64_t ld_out, bool train) {
        const NetLayout& n = w.net[which];
        HG_REQUIRE(M > 0 && M <= w.maxM, HGYM_E_SHAPE, "batch %d exceeds max_batch %lld", M, (long long)w.maxM);
        const LayerLayout& l0 = n.layer[0];
        const int64_t total = (int64_t)M * l0.K;
        hipLaunchKernelGGL((pack_rows_kernel<T>), dim3((int)std::min<int64_t>(ceil_div(total, 256), 4096)), dim3(256), 0, s, M, l0.K, x,
                           ldx, idx, at<T>(l0.X), (int64_t)l0.Kp);
        HG_CHECK_LAUNCH("pack_rows_kernel");
        const int Mp = (int)round_up(M, w.SE);
        for (int l = 0; l < n.L; ++l) {
            const LayerLayout& y = n.layer[l];
            const bool last = l == n.L - 1;
            if (train) {
                hipLaunchKernelGGL((transpose_kernel<T>), dim3(ceil_div(Mp, 64), ceil_div(y.K, 64)), dim3(256), 0, s, M, Mp, y.K,
                                   at<T>(y.X), (int64_t)y.Kp, at<T>(y.XT), w.Mp);
                HG_CHECK_LAUNCH("transpose_kernel");
            }
            GemmArgs g;
            memset(&g, 0, sizeof(g));
            g.A = at<T>(y.X);
            g.lda = y.Kp;
            g.rowsA = M;
            g.B = at<T>(y.Wp);
            g.ldb = y.Kp;
            g.rowsB = y.N16;
            g.M = M;
            g.N = y.N;
            g.K = y.Kp;
            g.bias = bias_in(which, l);
            if (last) {
                g.Cf = y_out;
                g.ldcf = ld_out;
            } else {
                g.act = ACT_APPLY;
                g.fn = w.act;
                g.Ct = at<T>(n.layer[l + 1].X);
                g.ldct = n.layer[l + 1].Kp;
            }
            const int32_t rc = launch_gemm<T>(g, 1, s);
            if (rc < 0) return rc;
        }
        return HGYM_OK;
    }

    // backward of one net given dY / dYT of its last layer already in the workspace
    int32_t backward(int which, int M) {
        const NetLayout& n = w.net[which];
        const int Mp = (int)round_up(M, w.SE);
        for (int l = n.L - 1; l >= 0; --l) {
            const LayerLayout& y = n.layer[l];
            {   // dW_l[N][K] = sum_m dY[m][n] * X[m][k]  (contraction over the batch, split-K slabs)
                GemmArgs g;
                memset(&g, 0, sizeof(g));
                g.A = at<T>(y.dYT);
                g.lda = w.Mp;
                g.rowsA = y.N16;
                g.B = at<T>(y.XT);
                g.ldb = w.Mp;
                g.rowsB = y.K16;
                g.M = y.N;
                g.N = y.K;
                g.K = Mp;
                g.Cf = at<float>(w.slabs) + y.w_off;
                g.ldcf = y.K;
                g.slab_stride = w.Ps;
                const int want = split_count(y, Mp);
                const int32_t got = launch_gemm<T>(g, want, s);
                if (got < 0) return got;
                HG_REQUIRE(got == want, HGYM_E_LAUNCH, "split-K mismatch %d vs %d", got, want);
                int per = 0;
                const int rs = rowsum_splits(Mp, &per);
                hipLaunchKernelGGL((rowsum_kernel<T>), dim3(rs, y.N), dim3(256), 0, s, Mp, per, at<T>(y.dYT), w.Mp,
                                   at<float>(w.slabs) + y.b_off, w.Ps);
                HG_CHECK_LAUNCH("rowsum_kernel");
            }
            if (l > 0) {   // dX = (dY * W) .* f'(z), from X_l = f(z)  -> dY of layer l-1
                const LayerLayout& p = n.layer[l - 1];
                GemmArgs g;
                memset(&g, 0, sizeof(g));
                g.A = at<T>(y.dY);
                g.lda = y.Ncp;
                g.rowsA = M;
                g.B = at<T>(y.WTp);
                g.ldb = y.Ncp;
                g.rowsB = y.K16;
                g.M = M;
                g.N = y.K;
                g.K = y.Ncp;
                g.aux = at<T>(y.X);
                g.ldaux = y.Kp;
                g.fn = w.act;
                g.Ct = at<T>(p.dY);
                g.ldct = p.Ncp;
                const int32_t rc = launch_gemm<T>(g, 1, s);
                if (rc < 0) return rc;
                hipLaunchKernelGGL((transpose_kernel<T>), dim3(ceil_div(Mp, 64), ceil_div(p.N, 64)), dim3(256), 0, s, M, Mp, p.N,
                                   at<T>(p.dY), (int64_t)p.Ncp, at<T>(p.dYT), w.Mp);
                HG_CHECK_LAUNCH("transpose_kernel");
            }
        }
        return HGYM_OK;
    }

    // Auxiliary (denoising) head, HgymNetConfig::aux_*: forward on the gathered observation rows, MSE against the target
    // columns of the gathered privileged rows, backward.  Leaves its weight and bias gradients in the split-K slabs; the
    // caller's slab reduction finishes them together with everything else.
    int32_t aux_grad(const HgymPPOConfig& ppo, const HgymBatch& b) {
        const NetLayout& n = w.net[2];
        const LayerLayout& last = n.layer[n.L - 1];
        const int B = b.B, No = last.N;
        float* y = at<float>(n.out_f32);
        int32_t rc = forward(2, B, b.obs, cfg.num_obs, b.idx, y, No, true);
        if (rc) return rc;
        const int Bp = (int)round_up(B, w.SE);
        hipLaunchKernelGGL((aux_mse_kernel<T>), dim3(ceil_div(Bp, 256)), dim3(256), 0, s, B, Bp, No, y, b.priv, (int64_t)cfg.num_priv,
                           cfg.aux_target_offset, b.idx, ppo.aux_coef, at<T>(last.dY), (int64_t)last.Ncp, at<T>(last.dYT), w.Mp,
                           net.opt_state);
        HG_CHECK_LAUNCH("aux_mse_kernel");
        return backward(2, B);
    }

    static LossSmooth loss_smooth(const ActorHead& h) { return {h.sm->target_next, h.sm->target_near, h.sm->next_weight, h.gT, h.gS}; }

    // part 1 (the second half of hgym_ppo_grad_part) has nothing left to do: part 0 does everything (the caller's first bucket goes out
    // complete, just later)
    int32_t grad(const HgymPPOConfig& ppo, const HgymBatch& b, int part, const ActorHead& h) {
        if (part == 1) return HGYM_OK;
        const int B = b.B, A = cfg.num_actions;
        float* mu = at<float>(w.net[0].out_f32);
        float* val = at<float>(w.net[1].out_f32);
        // (no zeroing of net.grads: ppo_scalars_kernel writes std's gradient, reduce_slabs_kernel every weight and bias segment)
        int32_t rc = head_prepass(*this, b, h);
        if (rc) return rc;
        rc = forward(0, B, b.obs, cfg.num_obs, b.idx, mu, A, true);
        if (rc) return rc;
        rc = forward(1, B, b.priv, cfg.num_priv, b.idx, val, 1, true);
        if (rc) return rc;
        const int Bp = (int)round_up(B, w.SE);
        const int nblocks = ceil_div(Bp, 256);
        HG_REQUIRE(nblocks <= MAX_LOSS_BLOCKS, HGYM_E_UNSUPPORTED, "minibatch %d too large for the loss partial buffer", B);
        // (head_partials holds 4 floats per 64 rows, a loss block covers 256 of the padded rows)
        HG_REQUIRE(!h.hp || nblocks <= (B + 63) / 64, HGYM_E_UNSUPPORTED, "%d loss blocks for B=%d: more than head_partials holds", nblocks, B);
        const LayerLayout& la = w.net[0].layer[w.net[0].L - 1];
        const LayerLayout& lc = w.net[1].layer[w.net[1].L - 1];
        LossArgs a;
        memset(&a, 0, sizeof(a));
        a.b = b;
        a.A = A;
        a.mu = mu;
        a.val = val;
        a.std_ = sigma_in();
        a.clip = ppo.clip_param;
        a.value_coef = ppo.value_loss_coef;
        a.entropy_coef = ppo.entropy_coef;
        a.dmu = at<T>(la.dY);
        a.ld_dmu = la.Ncp;
        a.dmuT = at<T>(la.dYT);
        a.ld_t = w.Mp;
        a.dval = at<T>(lc.dY);
        a.ld_dval = lc.Ncp;
        a.dvalT = at<T>(lc.dYT);
        a.Bp = Bp;
        a.partials = at<float>(w.partials);
        if (h.mirror()) {
            a.mt = b.mirror_target;
            a.m_src = b.mirror_act_src;
            a.m_sign = b.mirror_act_sign;
            a.m_g = h.m_g;
        }
        const bool bf16 = sizeof(T) == 2, unclipped = ppo.value_loss_unclipped != 0;
        prof_begin(HGYM_PROF_LOSS, s);
        if (unclipped) hipLaunchKernelGGL((ppo_loss_kernel<T, true>), dim3(nblocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((ppo_loss_kernel<T>), dim3(nblocks), dim3(256), 0, s, a);
        // behind it, the head's own kernel -- d mu with the head's terms, the LP_DBIAS_MU partials and the head's squared-error partials --, then its sums
        switch (h.kind) {
        case ActorHead::MIRROR_SMOOTH:      // fp32: the first two terms of d mu and LP_MIRROR are the mirror kernel's own, to the bit (hgym_loss_mirror_smooth.hip)
            if (!bf16) rc = launch_ppo_loss_mirror(a, false, unclipped, nblocks, s);
            if (!rc) rc = launch_ppo_loss_mirror_smooth(a, loss_smooth(h), h.hp, bf16, nblocks, s);
            break;
        case ActorHead::MIRROR: rc = launch_ppo_loss_mirror(a, bf16, unclipped, nblocks, s); break;
        case ActorHead::SMOOTH: rc = launch_ppo_loss_smooth(a, loss_smooth(h), bf16, nblocks, s); break;
        case ActorHead::GUIDE: rc = launch_ppo_loss_guide(a, LossGuide{h.gd->teacher_mu, h.gd->coef, h.inv2}, bf16, nblocks, s); break;
        case ActorHead::PLAIN: break;
        }
        if (!rc) rc = head_sums(h, nblocks, B, A, at<float>(w.partials), s);
        prof_end(HGYM_PROF_LOSS, s, (double)B * (4.0 * (5 * A + 6) + (double)sizeof(T) * (2 * A + 2)));      // (before the error return, as in bc_grad)
        if (rc) return rc;
        HG_CHECK_LAUNCH("ppo_loss_kernel");
        ScalArgs sc = {nblocks, B, A, 0, at<float>(w.partials), net.grads, nullptr, nullptr, net.grads + w.P, net.opt_state,
                       (double)ppo.beta1, (double)ppo.beta2, 0, 0, 0.0f, 0.0, 0.0, 1, grad_sigma()};
        if (h.mirror()) sc.mirror_sums = b.mirror_sums;      // (else null: off)
        hipLaunchKernelGGL(ppo_scalars_kernel, dim3(1), dim3(512), 0, s, sc);
        HG_CHECK_LAUNCH("ppo_scalars_kernel");
        rc = backward(0, B);
        if (rc) return rc;
        rc = backward(1, B);
        if (rc) return rc;
        if (w.nnets > 2) {
            rc = aux_grad(ppo, b);
            if (rc) return rc;
        }
        const SegTable tab = segments(Bp);
        hipLaunchKernelGGL(reduce_slabs_kernel, dim3(RSN_X, tab.n), dim3(256), 0, s, tab, w.Ps, at<float>(w.slabs), net.grads, net.opt_state);
        HG_CHECK_LAUNCH("reduce_slabs_kernel");
        return HGYM_OK;
    }

    // hgym_bc_grad: the actor's forward, bc_loss_kernel, the actor's backward, the actor's slab sums
    int32_t bc_grad(const HgymBCConfig& bc, const HgymBatch& b, const float* target, double* sums) {
        const int B = b.B, A = cfg.num_actions;
        float* mu = at<float>(w.net[0].out_f32);
        int32_t rc = bc_zero_grads();
        if (rc) return rc;
        rc = forward(0, B, b.obs, cfg.num_obs, b.idx, mu, A, true);
        if (rc) return rc;
        const int Bp = (int)round_up(B, w.SE);
        const int nblocks = ceil_div(Bp, 256);
        HG_REQUIRE(nblocks <= MAX_LOSS_BLOCKS, HGYM_E_UNSUPPORTED, "minibatch %d too large for the loss partial buffer", B);
        const LayerLayout& la = w.net[0].layer[w.net[0].L - 1];
        BcLossArgs a;
        memset(&a, 0, sizeof(a));
        a.mu = mu;
        a.target = target;
        a.idx = b.idx;
        a.B = B;
        a.Bp = Bp;
        a.A = A;
        a.dmu = at<T>(la.dY);
        a.ld_dmu = la.Ncp;
        a.dmuT = at<T>(la.dYT);
        a.ld_t = w.Mp;
        a.inv = 1.0f / ((float)B * (float)A);
        a.delta = bc.huber_delta;
        a.huber = bc.loss_type == HGYM_BC_HUBER;
        a.partials = at<float>(w.partials);
        rc = launch_bc_loss(a, sizeof(T) == 2, nblocks, s);
        if (rc) return rc;
        const BcScalArgs sc = {nblocks, B, A, at<float>(w.partials), nullptr, net.opt_state, sums};
        rc = launch_bc_scalars(sc, s);
        if (rc) return rc;
        rc = backward(0, B);
        if (rc) return rc;
        return bc_reduce_actor(Bp);
    }

    // the critic's forward and vf_loss_kernel: d V and its two partials are in place afterwards
    int32_t vf_head(const HgymVFConfig& vf, const HgymBatch& b, int Bp, int nblocks) {
        const int B = b.B;
        float* val = at<float>(w.net[1].out_f32);
        const int32_t rc = forward(1, B, b.priv, cfg.num_priv, b.idx, val, 1, true);
        if (rc) return rc;
        const LayerLayout& lc = w.net[1].layer[w.net[1].L - 1];
        VfLossArgs a;
        memset(&a, 0, sizeof(a));
        a.val = val;
        a.values = b.values;
        a.returns = b.returns;
        a.idx = b.idx;
        a.B = B;
        a.Bp = Bp;
        a.dval = at<T>(lc.dY);
        a.ld_dval = lc.Ncp;
        a.dvalT = at<T>(lc.dYT);
        a.clip = vf.clip_param;
        a.value_coef = vf.value_coef;
        a.partials = at<float>(w.partials);
        return launch_vf_loss(a, sizeof(T) == 2, vf.unclipped != 0, nblocks, s);
    }

    // hgym_vf_grad: the critic's forward, vf_loss_kernel, the scalars, the critic's backward, the critic's slab sums
    int32_t vf_grad(const HgymVFConfig& vf, const HgymBatch& b, double* sums) {
        const int B = b.B;
        const int Bp = (int)round_up(B, w.SE);
        const int nblocks = ceil_div(Bp, 256);
        HG_REQUIRE(nblocks <= MAX_LOSS_BLOCKS, HGYM_E_UNSUPPORTED, "minibatch %d too large for the loss partial buffer", B);
        int32_t rc = vf.keep_others ? HGYM_OK : bc_zero_grads();
        if (rc) return rc;
        rc = vf_head(vf, b, Bp, nblocks);
        if (rc) return rc;
        const VfScalArgs sc = {nblocks, B, cfg.num_actions, at<float>(w.partials), nullptr, net.opt_state, sums, vf.keep_others, nullptr, nullptr};
        rc = launch_vf_scalars(sc, s);
        if (rc) return rc;
        rc = backward(1, B);
        if (rc) return rc;
        return vf_reduce_critic(Bp);
    }

    // hgym_bc_vf_grad: both forwards, both heads, ONE scalars workgroup, both backwards, ONE slab pass over the actor and the critic
    int32_t bc_vf_grad(const HgymBCConfig& bc, const HgymVFConfig& vf, const HgymBatch& b, const float* target, double* bc_sums, double* vf_sums) {
        const int B = b.B, A = cfg.num_actions;
        float* mu = at<float>(w.net[0].out_f32);
        const int Bp = (int)round_up(B, w.SE);
        const int nblocks = ceil_div(Bp, 256);
        HG_REQUIRE(nblocks <= MAX_LOSS_BLOCKS, HGYM_E_UNSUPPORTED, "minibatch %d too large for the loss partial buffer", B);
        int32_t rc = bc_zero_grads();
        if (rc) return rc;
        rc = forward(0, B, b.obs, cfg.num_obs, b.idx, mu, A, true);
        if (rc) return rc;
        const LayerLayout& la = w.net[0].layer[w.net[0].L - 1];
        BcLossArgs a;
        memset(&a, 0, sizeof(a));
        a.mu = mu;
        a.target = target;
        a.idx = b.idx;
        a.B = B;
        a.Bp = Bp;
        a.A = A;
        a.dmu = at<T>(la.dY);
        a.ld_dmu = la.Ncp;
        a.dmuT = at<T>(la.dYT);
        a.ld_t = w.Mp;
        a.inv = 1.0f / ((float)B * (float)A);
        a.delta = bc.huber_delta;
        a.huber = bc.loss_type == HGYM_BC_HUBER;
        a.partials = at<float>(w.partials);
        rc = launch_bc_loss(a, sizeof(T) == 2, nblocks, s);
        if (rc) return rc;
        rc = vf_head(vf, b, Bp, nblocks);
        if (rc) return rc;
        const VfScalArgs sc = {nblocks, B, A, at<float>(w.partials), nullptr, net.opt_state, vf_sums, 0, nullptr, bc_sums};
        rc = launch_vf_scalars(sc, s);
        if (rc) return rc;
        rc = backward(0, B);
        if (rc) return rc;
        rc = backward(1, B);
        if (rc) return rc;
        return bc_vf_reduce(Bp);
    }

    int32_t act(int M, const float* obs, const float* priv, const float* z, uint64_t seed, const int64_t* step, float* actions, float* mu,
                float* sigma, float* logp, float* values, const FinArgs* fin, const HgymObsShadow* sh) {
        HG_REQUIRE(!sh || (!sh->obs && !sh->priv), HGYM_E_UNSUPPORTED, "the observation shadow exists on the fused bf16 path only (hgym_net_shadow_ld = 0 here)");
        if (fin) {     // the postponed finaliser as its own (tiny) launch
            hipLaunchKernelGGL(fin_only_kernel, dim3(1), dim3(1024), 0, s, *fin);
            HG_CHECK_LAUNCH("fin_only_kernel");
        }
        int32_t rc = forward(0, M, obs, cfg.num_obs, nullptr, mu, cfg.num_actions, false);
        if (rc) return rc;
        rc = forward(1, M, priv, cfg.num_priv, nullptr, values, 1, false);
        if (rc) return rc;
        hipLaunchKernelGGL(act_sample_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, s, M, cfg.num_actions, mu, sigma_in(), z, seed, step,
                           actions, sigma, logp);
        HG_CHECK_LAUNCH("act_sample_kernel");
        return HGYM_OK;
    }

    // the critic over M rows in pieces of at most max_batch (a multiple of 64 rows each when max_batch is at least 64)
    int32_t critic_values(int64_t M, const float* priv, float* values, const HgymObsShadow* sh) {
        HG_REQUIRE(!sh || !sh->priv, HGYM_E_UNSUPPORTED, "the observation shadow exists on the fused bf16 path only");
        const int64_t piece = w.maxM < 64 ? w.maxM : w.maxM / 64 * 64;
        for (int64_t m0 = 0; m0 < M; m0 += piece) {
            const int32_t rc = forward(1, (int)std::min<int64_t>(piece, M - m0), priv + m0 * cfg.num_priv, cfg.num_priv, nullptr, values + m0, 1,
                                       false);
            if (rc) return rc;
        }
        return HGYM_OK;
    }

    int32_t apply(const HgymPPOConfig& ppo) { return NetBase::apply<T>(ppo, false); }
    int32_t sync_shadow() { return NetBase::sync_shadow<T>(); }
    int32_t norm_refold() { return NetBase::norm_refold<T>(); }
};

// The fused bf16 path (hgym_fused.hpp): the actor and the critic, and the auxiliary head when it has the fused layout too, through
// mlp_fwd_kernel, mlp_fb_kernel and dw_kernel_rs.  An auxiliary head that does not fit those kernels takes the layer-by-layer path.
struct FusedPath : NetBase {
    GemmPath<__bf16> aux;

    explicit FusedPath(const NetBase& b) : NetBase(b), aux{b} {}

    struct SampleOut {
        const float* z; uint64_t seed; const int64_t* step; float* actions; float* sigma; float* logp;
    };

    FusedNet fused_net(int which, const NetIO& io) const {
        FusedNet f;
        memset(&f, 0, sizeof(f));
        const NetLayout& n = w.net[which];
        for (int l = 0; l < 4; ++l) {
            const LayerLayout& y = n.layer[l];
            FusedLayer& d = f.layer[l];
            d.Wf = at<u32x4>(y.Wf);
            d.WTf = at<u32x4>(y.WTf);
            d.bias = bias_in(which, l);
            d.K = y.K;
            d.N = y.N;
            d.KB = y.KBf;
            d.KR = y.KRf;
            d.NB = y.NBf;
            d.NBB = y.NBBf;
        }
        f.x = io.x;
        f.ldx = io.ldx;
        f.X0 = at<__bf16>(n.X0b);
        for (int l = 0; l < 3; ++l) f.H[l] = at<__bf16>(n.Hb[l]);
        for (int l = 0; l < 4; ++l) f.dZ[l] = at<__bf16>(n.dZb[l]);
        f.out = io.out;
        f.ldo = io.ldo;
        return f;
    }

    template <int BM, int NW, int D, bool FIN>
    int32_t launch_fwd_k(const FwdArgs& a, int nets) {
        const size_t lds = fwd_lds(a, nets, BM);
        const int32_t rc_lds = ensure_dynamic_lds(reinterpret_cast<const void*>(&mlp_fwd_kernel<BM, NW, D, FIN>), lds, "mlp_fwd_kernel");
        if (rc_lds) return rc_lds;
        FwdArgs b = a;
        b.nets = nets;
        const int rows = nets + (FIN ? 1 : 0);          // + the finaliser's grid row (its workgroup 0 works, the rest exit)
        b.dbg = phase_buffer((int64_t)ceil_div(a.M, BM) * rows);
        hipLaunchKernelGGL((mlp_fwd_kernel<BM, NW, D, FIN>), dim3(ceil_div(a.M, BM), rows), dim3(NW * 64), lds, s, b);
        HG_CHECK_LAUNCH("mlp_fwd_kernel");
        return HGYM_OK;
    }
    template <int BM, int NW, int D>
    int32_t launch_fwd(const FwdArgs& a, int nets) {
        if (!act_is_elu1(w.act)) {      // the generic instantiation: one launch per net, the postponed finaliser as its own (tiny) launch
            if (a.fin.N > 0) {
                hipLaunchKernelGGL(fin_only_kernel, dim3(1), dim3(1024), 0, s, a.fin);
                HG_CHECK_LAUNCH("fin_only_kernel");
            }
            FwdArgs b = a;
            const int64_t tiles = ceil_div(a.M, BM);
            b.dbg = phase_buffer(tiles * nets);
            const int32_t rc = launch_mlp_fwd_act(b, nets, BM == 64, tiles, s);
            if (rc) return rc;
            HG_CHECK_LAUNCH("mlp_fwd_act_kernel");
            return HGYM_OK;
        }
        return a.fin.N > 0 ? launch_fwd_k<BM, NW, D, true>(a, nets) : launch_fwd_k<BM, NW, D, false>(a, nets);
    }

    // sh (policy launches, no row gather): net 0 / 1 also store the bf16 of their input rows as rows of sh->obs / sh->priv
    FwdArgs make_fwd_args(int first, int nets, int M, const NetIO io[3], const int64_t* idx, bool train, const SampleOut* smp,
                          const FinArgs* fin, const HgymObsShadow* sh = nullptr) const {
        FwdArgs a;
        memset(&a, 0, sizeof(a));
        for (int i = first; i < first + nets; ++i) a.net[i] = fused_net(i, io[i]);
        if (sh && !idx && !train) {
            if (first == 0 && sh->obs) { a.net[0].xs = (__bf16*)sh->obs; a.net[0].ldxs = sh->ld_obs; }
            if (first <= 1 && first + nets > 1 && sh->priv) { a.net[1].xs = (__bf16*)sh->priv; a.net[1].ldxs = sh->ld_priv; }
        }
        a.net0 = first;
        a.act = w.act;
        a.M = M;
        a.idx = idx;
        if (fin) a.fin = *fin;
        a.train = train ? 3 : 0;
        a.A = cfg.num_actions;
        a.std_ = sigma_in();
        if (smp) {
            a.sample = 1;
            a.z = smp->z;
            a.k0 = (uint32_t)smp->seed;
            a.k1 = (uint32_t)(smp->seed >> 32);
            a.step = smp->step;
            a.actions = smp->actions;
            a.sigma = smp->sigma;
            a.logp = smp->logp;
        }
        return a;
    }

    // forward of `nets` networks starting at `first` in ONE launch
    int32_t forward_nets(int first, int nets, int M, const NetIO io[3], const int64_t* idx, bool train, const SampleOut* smp,
                         const FinArgs* fin = nullptr, const HgymObsShadow* sh = nullptr) {
        HG_REQUIRE(M > 0 && M <= w.maxM, HGYM_E_SHAPE, "batch %d exceeds max_batch %lld", M, (long long)w.maxM);
        const int32_t rc_sh = check_shadow(w, sh);
        if (rc_sh) return rc_sh;
        const FwdArgs a = make_fwd_args(first, nets, M, io, idx, train, smp, fin, sh);
        const int pcls = train ? HGYM_PROF_MLP_FWD : HGYM_PROF_POLICY;
        prof_begin(pcls, s);
        // 32-row tiles x 8 waves (weight ring depth 4) while they fit the chip in one round (one workgroup per CU: 2 * M / 32
        // <= CUs, i.e. 4096 envs), 64-row tiles x 16 waves (depth 2) for the update and for larger rollouts; measured
        // alternatives (64 rows x 8 waves, 32-row tiles for the update, other depths) were equal or slower
        const int cus = device_cus() > 0 ? device_cus() : 256;
        // (32-row tiles two per CU at 8192 rows: collection 5.32 vs 3.82 ms, profiles/r03_envs8192_policy_tiles_ab.txt)
        const int32_t rc = (train || nets * ceil_div(M, 32) > cus) ? launch_fwd<64, 16, 2>(a, nets) : launch_fwd<32, 8, 4>(a, nets);
        double fl = 0.0;
        for (int i = first; i < first + nets; ++i)
            for (int l = 0; l < 4; ++l) fl += 2.0 * (double)M * w.net[i].layer[l].N * w.net[i].layer[l].K;   // algorithmic (unpadded) flops
        prof_end(pcls, s, fl);
        return rc;
    }

    int32_t forward(int which, int M, const float* x, int64_t ldx, const int64_t* idx, float* y_out, int64_t ld_out, bool train) {
        if (!w.net[which].fused) return aux.forward(which, M, x, ldx, idx, y_out, ld_out, train);
        NetIO io[3] = {};
        io[which] = {x, ldx, y_out, ld_out};
        return forward_nets(which, 1, M, io, idx, train, nullptr);
    }

    // all weight (and hidden bias) gradients of nets [0, nets): one launch, split-K slabs, plus the loss-scalar workgroup `sc`
    // (the auxiliary head, net 2, reads the ACTOR's bf16 copy of the gathered observation rows as its first-layer operand -- same
    // rows, same columns -- and every bias gradient of it is a column sum of dZ: its loss has no per-tile partial sums for them)
    // gb (mlp_fb_kernel<XB16> ran): the first-layer operands were never copied -- those products gather their rows by gb->idx from the
    // bf16 shadows
    // ride: the loss-scalar workgroup `sc` rides in the launch (false: hgym_bc_grad, whose scalars have a launch of their own)
    // first: the first net whose products are launched (1: a critic-only step); gmask: bit i set -- net i gathers from gb's shadow
    // (a cloning step with the critic decides it per net, as its two halves do)
    int32_t dw(int nets, int B, const ScalArgs& sc, const HgymBatch* gb, bool ride = true, int first = 0, unsigned gmask = ~0u) {
        const int Bp = (int)round_up(B, 64);
        DwArgs d;
        memset(&d, 0, sizeof(d));
        d.B = B;
        int tile = 0;
        double fl = 0.0;
        for (int i = first; i < nets; ++i)
            for (int l = 0; l < 4; ++l) {
                const NetLayout& n = w.net[i];
                const LayerLayout& y = n.layer[l];
                HG_REQUIRE(d.np < DW_MAX_PRODUCTS, HGYM_E_UNSUPPORTED, "too many weight-gradient products in one launch");
                DwProduct& p = d.p[d.np++];
                p.Z = at<__bf16>(n.dZb[l]);
                p.CBz = l < 3 ? y.N / 16 : 2 * y.NBBf;
                p.X = l == 0 ? at<__bf16>(w.net[i == 2 ? 0 : i].X0b) : at<__bf16>(n.Hb[l - 1]);
                p.CBx = l == 0 ? 2 * y.KBf : y.K / 16;
                if (l == 0 && gb && ((gmask >> i) & 1u)) {
                    p.X = (const __bf16*)(i == 1 ? gb->priv_bf16 : gb->obs_bf16);
                    p.gidx = gb->idx;
                    p.ldg = shadow_ld(w, i == 1 ? 1 : 0);
                    p.CBx = (int)(p.ldg / 16);
                }
                p.N = y.N;
                p.K = y.K;
                p.w_off = y.w_off;
                p.b_off = (l < 3 || i == 2) ? y.b_off : -1;
                p.tiles_n = ceil_div(y.N, DW_TILE_N);
                p.tiles_k = ceil_div(y.K, DW_TILE_K);
                p.tile0 = tile;
                tile += p.tiles_n * p.tiles_k;
                fl += 2.0 * (double)B * y.N * y.K;
            }
        d.total_tiles = tile;
        d.splits = w.dw_splits;
        d.steps_total = Bp / 32;
        d.steps_per_split = ceil_div(d.steps_total, w.dw_splits);
        d.slabs = at<float>(w.slabs);
        d.slab_stride = w.Ps;
        d.zeros = at<char>(w.zeros);
        d.sc = sc;
        d.scal_bid = ride ? tile * (int)round_up(w.dw_splits, 8) : -1;
        const int blocks = tile * (int)round_up(w.dw_splits, 8) + (ride ? 1 : 0);
        const int32_t rc_lds = ensure_dynamic_lds(reinterpret_cast<const void*>(&dw_kernel_rs<3>), DW_LDS_STAGES * DW_STAGE_BYTES, "dw_kernel_rs");
        if (rc_lds != HGYM_OK) return rc_lds;
        prof_begin(HGYM_PROF_DW, s);
        hipLaunchKernelGGL(dw_kernel_rs<3>, dim3(blocks), dim3(DW_THREADS), DW_LDS_STAGES * DW_STAGE_BYTES, s, d);
        prof_end(HGYM_PROF_DW, s, fl);
        HG_CHECK_LAUNCH("dw_kernel_rs");
        return HGYM_OK;
    }

    // The update tiles of a minibatch over nets [0, nets): what grad and bc_grad decide, check and fill in the same way.  Two steps,
    // because both launch something in between (the pre-passes; the zero fill) and plan_tiles' refusal comes before any launch.
    struct UpdateTiles {
        bool shadow;      // the tiles gather their rows from the bf16 shadows of the storage rows (HgymBatch.obs_bf16 / priv_bf16)
        int tiles;        // 64-row tiles per net
        size_t lds;       // dynamic LDS of the net that needs most
        FwdArgs fb;
        FbLoss fl;        // zero but for `partials`: the caller's head fills in what it reads
    };
    static const void* shadow_rows(const HgymBatch& b, int i) { return i == 1 ? b.priv_bf16 : b.obs_bf16; }

    // first: the first net of the tiles (1: the critic alone)
    int32_t plan_tiles(const HgymBatch& b, int nets, UpdateTiles* u, int first = 0) const {
        const int B = b.B;
        // bf16 shadows of the storage rows, every net's or none: gather 2 B per element, keep no operand copy
        u->shadow = b.num_rows > 0;
        for (int i = first; i < nets; ++i)
            u->shadow = u->shadow && shadow_rows(b, i) && b.num_rows * shadow_ld(w, i == 1 ? 1 : 0) * 2 < ((int64_t)1 << 32);
        // (128-row tiles on eight 256-register wavefronts -- round 4's mlp_fb2_kernel -- measured equal to slightly slower:
        // profiles/r04_fb2_128row_tiles_negative_result.txt; its source is profiles/r04_fb2_128row_kernel.patch; round 6 rebuilt the idea on role-specialised wavefronts at 64 and 128 rows: profiles/r06_fb3_role_specialised_wavefronts.txt.)
        const int tiles = (int)round_up(B, 64) / 64;
        HG_REQUIRE(tiles <= MAX_LOSS_BLOCKS, HGYM_E_UNSUPPORTED, "minibatch %d too large for the loss partial buffer", B);
        u->tiles = tiles;
        return HGYM_OK;
    }

    // kernel: the name that the LDS refusal gives
    int32_t fill_tiles(const HgymBatch& b, int nets, const NetIO io[3], const char* kernel, UpdateTiles* u, int first = 0) {
        FwdArgs& fb = u->fb;
        fb = make_fwd_args(first, nets - first, b.B, io, b.idx, true, nullptr, nullptr);
        if (nets > 2) fb.net[2].X0 = nullptr;       // the head's first-layer operand for the weight gradient is the actor's copy (dw)
        if (u->shadow) {
            uintptr_t bits = 0;
            for (int i = first; i < nets; ++i) bits |= (uintptr_t)shadow_rows(b, i);
            HG_REQUIRE((bits & 15) == 0, HGYM_E_BADARG, "observation shadows must be 16-byte aligned");
            for (int i = first; i < nets; ++i) {
                fb.net[i].xb = (const __bf16*)shadow_rows(b, i);
                fb.net[i].ldxb = shadow_ld(w, i == 1 ? 1 : 0);
                fb.net[i].X0 = nullptr;
            }
        }
        memset(&u->fl, 0, sizeof(u->fl));
        u->fl.partials = at<float>(w.partials);
        u->lds = 0;
        for (int i = first; i < nets; ++i)
            u->lds = std::max(u->lds, (size_t)fb_lds_bytes(fb.net[i]));       // the nets the kernel receives (fused_supported: same sum)
        HG_REQUIRE(u->lds <= FB_LDS_LIMIT, HGYM_E_UNSUPPORTED, "%s needs %zu bytes of LDS", kernel, u->lds);
        fb.nets = nets;
        fb.dbg = phase_buffer((int64_t)u->tiles * nets);
        return HGYM_OK;
    }

    // algorithmic (unpadded) flops of the update tiles of nets [0, nets): the forward and the dZ chain
    double tile_flops(int nets, int B) const {
        double flops = 0.0;
        for (int i = 0; i < nets; ++i) {
            for (int l = 0; l < 4; ++l) flops += 2.0 * (double)B * w.net[i].layer[l].N * w.net[i].layer[l].K;
            for (int l = 1; l < 4; ++l) flops += 2.0 * (double)B * w.net[i].layer[l].K * w.net[i].layer[l].N;
        }
        return flops;
    }

    // the actor's tiles with `head` in them, their own launch (hgym_fused.hpp: mlp_fb_head_kernel)
    template <class Head>
    int32_t launch_actor_head(const UpdateTiles& u, const Head& head) {
        return act_is_elu1(w.act) ? launch_mlp_fb_head<false, Head>(u.fb, u.fl, head, u.shadow, u.tiles, s)
                                  : launch_mlp_fb_head<true, Head>(u.fb, u.fl, head, u.shadow, u.tiles, s);
    }

    // the head records of the mirror loss and of the smoothness regulariser (`stage` is the launch's to set)
    static FbMirror fb_mirror(const HgymBatch& b, const ActorHead& h) { return {b.mirror_target, b.mirror_act_src, b.mirror_act_sign, h.m_g, 0}; }
    static FbSmooth fb_smooth(const ActorHead& h) { return {h.sm->target_next, h.sm->target_near, h.sm->next_weight, h.gT, h.gS, 0}; }

    // the tiles of nets [first, nets) through the kernels every net always had
    int32_t launch_rest(const UpdateTiles& u, bool unclipped, int nets, int first) {
        if (!act_is_elu1(w.act)) return launch_mlp_fb_act(u.fb, u.fl, u.shadow, unclipped, u.tiles, nets, s, first);
        FwdArgs rest = u.fb;      // (hgym_update.hip: the kernel's own code object)
        rest.net0 = first;
        rest.nets = nets - first;
        if (rest.dbg) rest.dbg += (int64_t)first * u.tiles * 8;      // phase stamps: behind the actor's slots
        return launch_mlp_fb(rest, u.fl, u.shadow, unclipped, u.tiles, nets - first, u.lds, s);
    }

    // part < 0: the whole minibatch gradient.  part 0 / 1: the two halves of hgym_ppo_grad_part -- 0 leaves std's and the actor's
    // gradient final, 1 the critic's, the auxiliary head's and the KL slot.
    int32_t grad(const HgymPPOConfig& ppo, const HgymBatch& b, int part, const ActorHead& h) {
        const int B = b.B, A = cfg.num_actions;
        const int64_t critic_off = w.net[1].layer[0].w_off;
        const int Mp = (int)round_up(B, w.SE);
        // In two parts (hgym_ppo_grad_part): part 0 runs everything up to and including ALL weight-gradient products and sums the
        // slabs of [std | actor]; part 1 only sums the rest.  (Until round 3 part 1 also launched the critic's products on their own:
        // two launches of 144 and 112 workgroups on 256 CUs, each as long as the full one -- 2 x 142 us against 178 us.)
        if (part == 1) return reduce_range(critic_off, w.P, Mp);
        const int nets = w.net[2].fused ? 3 : 2;      // the auxiliary head as a third grid row of the same launches
        UpdateTiles u;
        const int32_t rc_plan = plan_tiles(b, nets, &u);
        if (rc_plan) return rc_plan;
        const int32_t rc_pre = head_prepass(*this, b, h);
        if (rc_pre) return rc_pre;
        {   // forward + PPO loss + dZ chain of both nets: ONE launch (hgym_fused.hpp: mlp_fb_kernel)
            const NetIO io[3] = {{b.obs, cfg.num_obs, at<float>(w.net[0].out_f32), A},
                                 {b.priv, cfg.num_priv, at<float>(w.net[1].out_f32), 1},
                                 {b.obs, cfg.num_obs, nullptr, 0}};
            const int32_t rc_fill = fill_tiles(b, nets, io, "mlp_fb_kernel", &u);
            if (rc_fill) return rc_fill;
            FbLoss& fl = u.fl;
            fl.actions = b.actions;
            fl.old_mu = b.mu;
            fl.old_sigma = b.sigma;
            fl.values = b.values;
            fl.advantages = b.advantages;
            fl.returns = b.returns;
            fl.logp = b.logp;
            fl.clip = ppo.clip_param;
            fl.value_coef = ppo.value_loss_coef;
            fl.entropy_coef = ppo.entropy_coef;
            fl.aux_target = b.priv;
            fl.aux_ldt = cfg.num_priv;
            fl.aux_off = cfg.aux_target_offset;
            fl.aux_coef = ppo.aux_coef;
            prof_begin(HGYM_PROF_MLP_FWD, s);
            int32_t rc_fb = HGYM_OK;
            // a head of the actor's own: the actor's tiles through the kernels with it in their head (their own launch), then its sums, the rest from net 1 on
            switch (h.kind) {
            case ActorHead::MIRROR_SMOOTH: rc_fb = launch_actor_head(u, FbMirrorSmooth{fb_mirror(b, h), fb_smooth(h), h.hp, 0}); break;
            case ActorHead::MIRROR: rc_fb = launch_actor_head(u, fb_mirror(b, h)); break;
            case ActorHead::SMOOTH: rc_fb = launch_actor_head(u, fb_smooth(h)); break;
            case ActorHead::GUIDE: rc_fb = launch_actor_head(u, FbGuide{h.gd->teacher_mu, h.gd->coef, h.inv2, 0}); break;      // (the coefficient is read on the device)
            case ActorHead::PLAIN: break;
            }
            if (!rc_fb) rc_fb = head_sums(h, u.tiles, B, A, at<float>(w.partials), s);
            const int first = h.kind != ActorHead::PLAIN;      // the first net of the launches every net always had
            if (!rc_fb) rc_fb = launch_rest(u, ppo.value_loss_unclipped != 0, nets, first);
            prof_end(HGYM_PROF_MLP_FWD, s, tile_flops(nets, B));      // (before the error return, as in bc_grad)
            if (rc_fb) return rc_fb;
            HG_CHECK_LAUNCH("mlp_fb_kernel");
        }
        // the minibatch's loss scalars (per-tile partials -> opt_state, std / head-bias gradients, KL slot): one extra workgroup of
        // the weight-gradient launch that follows anyway (it needs nothing but the partials mlp_fb_kernel has just written)
        ScalArgs sc = {u.tiles, B, A, nets == 3 ? w.net[2].layer[3].N : 0, at<float>(w.partials), net.grads,
                             net.grads + w.net[0].layer[3].b_off, net.grads + w.net[1].layer[3].b_off, net.grads + w.P, net.opt_state,
                             (double)ppo.beta1, (double)ppo.beta2, prologue_in_grad(ppo) ? 1 : 0, ppo.adaptive_lr, ppo.desired_kl, ppo.lr_min,
                             ppo.lr_max, 1, grad_sigma()};
        if (h.mirror()) sc.mirror_sums = b.mirror_sums;      // (else null: off)
        int32_t rc = dw(nets, B, sc, u.shadow ? &b : nullptr);
        if (rc) return rc;
        if (w.nnets > 2 && nets == 2) {
            rc = aux.aux_grad(ppo, b);
            if (rc) return rc;
        }
        return part == 0 ? reduce_range(0, critic_off, Mp) : reduce_range(0, w.P, Mp);
    }

    // hgym_bc_grad: the actor's tiles with the regression head (forward, d mu, dZ chain: one launch), the scalars, the actor's four
    // weight-gradient products, the actor's slab sums
    int32_t bc_grad(const HgymBCConfig& bc, const HgymBatch& b, const float* target, double* sums) {
        const int B = b.B, A = cfg.num_actions;
        const int Mp = (int)round_up(B, w.SE);
        UpdateTiles u;
        int32_t rc = plan_tiles(b, 1, &u);
        if (rc) return rc;
        HG_REQUIRE(A != 12 || ((uintptr_t)target & 15) == 0, HGYM_E_BADARG, "hgym_bc_grad: target must be 16-byte aligned");
        rc = bc_zero_grads();
        if (rc) return rc;
        const NetIO io[3] = {{b.obs, cfg.num_obs, at<float>(w.net[0].out_f32), A}, {}, {}};
        rc = fill_tiles(b, 1, io, "mlp_fb_bc_kernel", &u);
        if (rc) return rc;
        const FbBC head = {target, 1.0f / ((float)B * (float)A), bc.huber_delta, bc.loss_type == HGYM_BC_HUBER ? 1 : 0};
        prof_begin(HGYM_PROF_MLP_FWD, s);
        rc = launch_actor_head(u, head);
        prof_end(HGYM_PROF_MLP_FWD, s, tile_flops(1, B));      // (before the error return: a refused launch must not leave the interval open)
        if (rc) return rc;
        HG_CHECK_LAUNCH("mlp_fb_bc_kernel");
        const BcScalArgs sc = {u.tiles, B, A, at<float>(w.partials), net.grads + w.net[0].layer[3].b_off, net.opt_state, sums};
        rc = launch_bc_scalars(sc, s);
        if (rc) return rc;
        ScalArgs none;
        memset(&none, 0, sizeof(none));
        rc = dw(1, B, none, u.shadow ? &b : nullptr, false);
        if (rc) return rc;
        return bc_reduce_actor(Mp);
    }

    // The critic's tiles of a critic-only step, through the kernels the critic always had (launch_rest from net 1 on): planned and
    // filled (vf_tiles, before anything is launched), then launched (vf_launch).
    int32_t vf_tiles(const HgymVFConfig& vf, const HgymBatch& b, UpdateTiles* u) {
        int32_t rc = plan_tiles(b, 2, u, 1);
        if (rc) return rc;
        const NetIO io[3] = {{}, {b.priv, cfg.num_priv, at<float>(w.net[1].out_f32), 1}, {}};
        rc = fill_tiles(b, 2, io, "mlp_fb_kernel", u, 1);
        if (rc) return rc;
        FbLoss& fl = u->fl;
        fl.values = (vf.unclipped && !b.values) ? b.returns : b.values;      // (the unclipped tile still loads the old value and drops it)
        fl.returns = b.returns;
        fl.clip = vf.clip_param;
        fl.value_coef = vf.value_coef;
        return HGYM_OK;
    }
    int32_t vf_launch(const HgymVFConfig& vf, const UpdateTiles& u, int B) {
        double flops = 0.0;
        for (int l = 0; l < 4; ++l) flops += (l > 0 ? 4.0 : 2.0) * (double)B * w.net[1].layer[l].N * w.net[1].layer[l].K;
        prof_begin(HGYM_PROF_MLP_FWD, s);
        const int32_t rc = launch_rest(u, vf.unclipped != 0, 2, 1);
        prof_end(HGYM_PROF_MLP_FWD, s, flops);      // (before the error return, as in bc_grad)
        if (rc) return rc;
        HG_CHECK_LAUNCH("mlp_fb_kernel");
        return HGYM_OK;
    }

    // hgym_vf_grad: the critic's tiles, the scalars, the critic's four weight-gradient products, the critic's slab sums
    int32_t vf_grad(const HgymVFConfig& vf, const HgymBatch& b, double* sums) {
        const int B = b.B;
        const int Mp = (int)round_up(B, w.SE);
        UpdateTiles u;
        int32_t rc = vf_tiles(vf, b, &u);
        if (rc) return rc;
        rc = vf.keep_others ? HGYM_OK : bc_zero_grads();
        if (rc) return rc;
        rc = vf_launch(vf, u, B);
        if (rc) return rc;
        const VfScalArgs sc = {u.tiles, B, cfg.num_actions, at<float>(w.partials), net.grads + w.net[1].layer[3].b_off, net.opt_state, sums,
                               vf.keep_others, nullptr, nullptr};
        rc = launch_vf_scalars(sc, s);
        if (rc) return rc;
        ScalArgs none;
        memset(&none, 0, sizeof(none));
        rc = dw(2, B, none, u.shadow ? &b : nullptr, false, 1);
        if (rc) return rc;
        return vf_reduce_critic(Mp);
    }

    // hgym_bc_vf_grad: the actor's tiles with the regression head, the critic's plain tiles, ONE scalars workgroup, ONE weight-gradient launch
    // with the eight products, ONE slab pass.  Each net decides on its shadow as its own call would.
    int32_t bc_vf_grad(const HgymBCConfig& bc, const HgymVFConfig& vf, const HgymBatch& b, const float* target, double* bc_sums, double* vf_sums) {
        const int B = b.B, A = cfg.num_actions;
        const int Mp = (int)round_up(B, w.SE);
        UpdateTiles ua, uc;
        int32_t rc = plan_tiles(b, 1, &ua);
        if (rc) return rc;
        HG_REQUIRE(A != 12 || ((uintptr_t)target & 15) == 0, HGYM_E_BADARG, "hgym_bc_vf_grad: target must be 16-byte aligned");
        rc = vf_tiles(vf, b, &uc);
        if (rc) return rc;
        const NetIO io[3] = {{b.obs, cfg.num_obs, at<float>(w.net[0].out_f32), A}, {}, {}};
        rc = fill_tiles(b, 1, io, "mlp_fb_bc_kernel", &ua);
        if (rc) return rc;
        rc = bc_zero_grads();
        if (rc) return rc;
        const FbBC head = {target, 1.0f / ((float)B * (float)A), bc.huber_delta, bc.loss_type == HGYM_BC_HUBER ? 1 : 0};
        prof_begin(HGYM_PROF_MLP_FWD, s);
        rc = launch_actor_head(ua, head);
        prof_end(HGYM_PROF_MLP_FWD, s, tile_flops(1, B));
        if (rc) return rc;
        HG_CHECK_LAUNCH("mlp_fb_bc_kernel");
        rc = vf_launch(vf, uc, B);
        if (rc) return rc;
        const VfScalArgs sc = {ua.tiles, B, A, at<float>(w.partials), net.grads + w.net[1].layer[3].b_off, net.opt_state, vf_sums, 0,
                               net.grads + w.net[0].layer[3].b_off, bc_sums};
        rc = launch_vf_scalars(sc, s);
        if (rc) return rc;
        ScalArgs none;
        memset(&none, 0, sizeof(none));
        const unsigned gmask = (ua.shadow ? 1u : 0u) | (uc.shadow ? 2u : 0u);
        rc = dw(2, B, none, gmask ? &b : nullptr, false, 0, gmask);
        if (rc) return rc;
        return bc_vf_reduce(Mp);
    }

    int32_t act(int M, const float* obs, const float* priv, const float* z, uint64_t seed, const int64_t* step, float* actions, float* mu,
                float* sigma, float* logp, float* values, const FinArgs* fin, const HgymObsShadow* sh) {
        const NetIO io[3] = {{obs, cfg.num_obs, mu, cfg.num_actions}, {priv, cfg.num_priv, values, 1}, {}};
        const SampleOut smp = {z, seed, step, actions, sigma, logp};
        return forward_nets(0, 2, M, io, nullptr, false, &smp, fin, sh);
    }

    // the critic over M rows in pieces of at most max_batch (a multiple of 64 rows each: whole tiles; max_batch itself below 64), the
    // shadow's priv rows written by the tiles that read them
    int32_t critic_values(int64_t M, const float* priv, float* values, const HgymObsShadow* sh) {
        const int64_t piece = w.maxM < 64 ? w.maxM : w.maxM / 64 * 64;
        for (int64_t m0 = 0; m0 < M; m0 += piece) {
            const NetIO io[3] = {{}, {priv + m0 * cfg.num_priv, cfg.num_priv, values + m0, 1}, {}};
            HgymObsShadow s1 = {nullptr, 0, nullptr, 0};
            if (sh && sh->priv) {
                s1.priv = (char*)sh->priv + m0 * sh->ld_priv * 2;
                s1.ld_priv = sh->ld_priv;
            }
            const int32_t rc = forward_nets(1, 1, (int)std::min<int64_t>(piece, M - m0), io, nullptr, false, nullptr, nullptr,
                                            (sh && sh->priv) ? &s1 : nullptr);
            if (rc) return rc;
        }
        return HGYM_OK;
    }

    // One rank with grad_norm_ready: the loss-scalar workgroup that rides in the weight-gradient launch has already taken the
    // learning-rate decision and prepared Adam's step scalars (ScalArgs::do_prologue); hgym_ppo_apply then starts with Adam.
    bool prologue_in_grad(const HgymPPOConfig& ppo) const { return ppo.world_size <= 1 && ppo.grad_norm_ready != 0; }

    int32_t apply(const HgymPPOConfig& ppo) { return NetBase::apply<__bf16>(ppo, prologue_in_grad(ppo)); }
    int32_t sync_shadow() { return NetBase::sync_shadow<__bf16>(); }
    int32_t norm_refold() { return NetBase::norm_refold<__bf16>(); }
};

static int32_t check_net(const HgymNetConfig* cfg, const HgymNet* net, WsLayout* w) {
    HG_REQUIRE(cfg && net, HGYM_E_BADARG, "null net config / net");
    const int32_t rc = ws_layout(cfg, w);
    if (rc) return rc;
    HG_REQUIRE(net->params && net->workspace, HGYM_E_BADARG, "null params / workspace");
    HG_REQUIRE(((uintptr_t)net->workspace & 255) == 0, HGYM_E_BADARG, "workspace must be 256-byte aligned");
    HG_REQUIRE(((uintptr_t)net->norm & 255) == 0, HGYM_E_BADARG, "HgymNet.norm must be 256-byte aligned");
    return HGYM_OK;
}

static NetBase net_base(const HgymNetConfig* cfg, const HgymNet* net, const WsLayout& w, hipStream_t s) {
    NetBase b{*cfg, *net, w, s, (char*)net->workspace, {}};
    if (net->norm) norm_layout(cfg, &b.nl);
    return b;
}

static int32_t check_ppo(const HgymPPOConfig* ppo) {
    HG_REQUIRE(ppo, HGYM_E_BADARG, "null ppo");
    HG_REQUIRE(ppo->value_loss_unclipped == 0 || ppo->value_loss_unclipped == 1, HGYM_E_BADARG,
               "HgymPPOConfig.value_loss_unclipped=%d (0: clipped value loss, 1: unclipped)", ppo->value_loss_unclipped);
    // (written so that a NaN fails it)
    HG_REQUIRE(ppo->mirror_coef >= 0.0f && ppo->mirror_coef < INFINITY, HGYM_E_BADARG,
               "HgymPPOConfig.mirror_coef=%g must be finite and >= 0 (0: no mirror loss)", (double)ppo->mirror_coef);
    return HGYM_OK;
}

static int32_t check_batch(const WsLayout& w, const HgymPPOConfig* ppo, const HgymBatch* b) {
    HG_REQUIRE(b, HGYM_E_BADARG, "null batch");
    if (ppo->mirror_coef > 0.0f) {
        HG_REQUIRE(b->pair_idx && b->mirror_act_src && b->mirror_act_sign && b->mirror_target && b->mirror_sums, HGYM_E_BADARG,
                   "HgymPPOConfig.mirror_coef > 0 needs HgymBatch.pair_idx, mirror_act_src, mirror_act_sign, mirror_target and mirror_sums");
        HG_REQUIRE(((uintptr_t)b->mirror_target & 15) == 0, HGYM_E_BADARG, "HgymBatch.mirror_target must be 16-byte aligned");
        HG_REQUIRE(((uintptr_t)b->mirror_sums & 7) == 0 && ((uintptr_t)b->pair_idx & 7) == 0, HGYM_E_BADARG,
                   "HgymBatch.mirror_sums / pair_idx must be 8-byte aligned");
    }
    HG_REQUIRE(b->obs && b->priv && b->actions && b->values && b->advantages && b->returns && b->logp && b->mu && b->sigma && b->idx,
               HGYM_E_BADARG, "null batch tensor");
    HG_REQUIRE(b->B > 0 && b->B <= w.maxM, HGYM_E_SHAPE, "minibatch %d exceeds max_batch %lld", b->B, (long long)w.maxM);
    return HGYM_OK;
}

// The one place that picks a runner: the fused path when ws_layout gave the actor and the critic the fused layout, else the
// layer-by-layer path in the configured precision.  `f` receives the runner; check_net's failures return before it runs.
template <class F>
static int32_t run(const HgymNetConfig* cfg, const HgymNet* net, void* stream, F&& f) {
    WsLayout w;
    const int32_t rc = check_net(cfg, net, &w);
    if (rc) return rc;
    const NetBase b = net_base(cfg, net, w, (hipStream_t)stream);
    if (w.net[0].fused) {
        FusedPath R(b);
        return f(R);
    }
    if (cfg->precision == HGYM_F32) {
        GemmPath<float> R{b};
        return f(R);
    }
    GemmPath<__bf16> R{b};
    return f(R);
}

// For hgym_rollout.hip (the fused policy + env step lives in a translation unit of its own: it also contains the env
// arithmetic, which is built with -ffp-contract=off): the FwdArgs record of one PPO.act launch over the actor and the critic
// with 32-row tiles, and the dynamic LDS those tiles need.  Fails unless the fused bf16 path serves this configuration with
// XBot-L's first hidden widths (actor 512, critic 768: the instantiations the rollout kernel carries).
int32_t rollout_fwd_args(const HgymNetConfig* cfg, const HgymNet* net, int M, const float* obs, const float* priv, uint64_t seed,
                         const int64_t* step, float* actions, float* mu, float* sigma, float* logp, float* values, FwdArgs* out,
                         size_t* lds_bytes, const HgymObsShadow* sh, const float* z) {
    WsLayout w;
    int32_t rc = check_net(cfg, net, &w);
    if (rc) return rc;
    HG_REQUIRE(w.net[0].fused, HGYM_E_UNSUPPORTED, "the fused rollout step needs the bf16 fused path");
    HG_REQUIRE(M > 0 && M <= w.maxM, HGYM_E_SHAPE, "batch %d exceeds max_batch %lld", M, (long long)w.maxM);
    HG_REQUIRE(cfg->actor_dims[1] == 512 && cfg->critic_dims[1] == 768, HGYM_E_UNSUPPORTED,
               "fused rollout step: first hidden widths 512 / 768 (XBot-L) only, not %d / %d", cfg->actor_dims[1], cfg->critic_dims[1]);
    rc = check_shadow(w, sh);
    if (rc) return rc;
    const FusedPath R(net_base(cfg, net, w, nullptr));
    const NetIO io[3] = {{obs, cfg->num_obs, mu, cfg->num_actions}, {priv, cfg->num_priv, values, 1}, {}};
    const FusedPath::SampleOut smp = {z, seed, step, actions, sigma, logp};
    *out = R.make_fwd_args(0, 2, M, io, nullptr, false, &smp, nullptr, sh);
    out->nets = 2;
    *lds_bytes = fwd_lds(*out, 2, 32);
    return HGYM_OK;
}

// The evaluation launch's tile (hgym_rollout_eval_step): the actor alone, no sampling epilogue, its head outputs written to `actions`.
int32_t rollout_eval_fwd_args(const HgymNetConfig* cfg, const HgymNet* net, int M, const float* obs, float* actions, FwdArgs* out,
                              size_t* lds_bytes) {
    WsLayout w;
    int32_t rc = check_net(cfg, net, &w);
    if (rc) return rc;
    HG_REQUIRE(w.net[0].fused, HGYM_E_UNSUPPORTED, "the fused evaluation step needs the bf16 fused path");
    HG_REQUIRE(M > 0 && M <= w.maxM, HGYM_E_SHAPE, "batch %d exceeds max_batch %lld", M, (long long)w.maxM);
    HG_REQUIRE(cfg->actor_dims[1] == 512, HGYM_E_UNSUPPORTED, "fused evaluation step: first hidden width 512 (XBot-L) only, not %d",
               cfg->actor_dims[1]);
    const FusedPath R(net_base(cfg, net, w, nullptr));
    const NetIO io[3] = {{obs, cfg->num_obs, actions, cfg->num_actions}, {}, {}};
    *out = R.make_fwd_args(0, 1, M, io, nullptr, false, nullptr, nullptr, nullptr);
    out->nets = 1;
    *lds_bytes = fwd_lds(*out, 1, 32);
    return HGYM_OK;
}

// For hgym_diag.hip: sigma_src behind the configuration check.
int32_t net_sigma_src(const HgymNetConfig* cfg, const HgymNet* net, const float** out) {
    WsLayout w;
    const int32_t rc = check_net(cfg, net, &w);
    if (rc) return rc;
    *out = sigma_src(w, *net);
    return HGYM_OK;
}

// For hgym_norm.hip: the first layers of the nets in the flat parameter vector, behind the configuration check.
int32_t net_first_layers(const HgymNetConfig* cfg, NormFirst out[3], int* nnets) {
    WsLayout w;
    const int32_t rc = ws_layout(cfg, &w);
    if (rc) return rc;
    for (int i = 0; i < w.nnets; ++i) out[i] = NormFirst{w.net[i].layer[0].w_off, w.net[i].layer[0].b_off, w.net[i].layer[0].N, w.net[i].layer[0].K};
    *nnets = w.nnets;
    return HGYM_OK;
}

int32_t net_norm_refold(const HgymNetConfig* cfg, const HgymNet* net, void* stream) {
    return run(cfg, net, stream, [](auto& R) { return R.norm_refold(); });
}

}  // namespace hgym

using namespace hgym;

extern "C" {

int64_t hgym_net_param_count(const HgymNetConfig* cfg) {
    WsLayout w;
    if (ws_layout(cfg, &w)) return -1;
    return w.P;
}

int64_t hgym_net_workspace_bytes(const HgymNetConfig* cfg) {
    WsLayout w;
    if (ws_layout(cfg, &w)) return -1;
    return w.total_bytes;
}

int64_t hgym_net_sigma_offset(const HgymNetConfig* cfg) {
    WsLayout w;
    if (ws_layout(cfg, &w)) return -2;
    return w.sigma;      // -1: HGYM_STD_SCALAR
}

int32_t hgym_net_sync_shadow(const HgymNetConfig* cfg, const HgymNet* net, void* stream) {
    return run(cfg, net, stream, [](auto& R) { return R.sync_shadow(); });
}

int32_t hgym_mlp_forward(const HgymNetConfig* cfg, const HgymNet* net, int32_t which, int32_t M, const float* x, int64_t ldx, float* y,
                         void* stream) {
    return run(cfg, net, stream, [&](auto& R) -> int32_t {
        HG_REQUIRE(which == 0 || which == 1 || (which == 2 && cfg->aux_layers > 0), HGYM_E_BADARG, "which=%d", which);
        HG_REQUIRE(x && y, HGYM_E_BADARG, "null x / y");
        const int nout = which == 0 ? cfg->num_actions : (which == 1 ? 1 : cfg->aux_dims[cfg->aux_layers]);
        return R.forward(which, M, x, ldx, nullptr, y, nout, false);
    });
}

int32_t hgym_critic_values(const HgymNetConfig* cfg, const HgymNet* net, int64_t M, const float* priv, float* values,
                           const HgymObsShadow* shadow, void* stream) {
    return run(cfg, net, stream, [&](auto& R) -> int32_t {
        HG_REQUIRE(M > 0 && priv && values, HGYM_E_BADARG, "M=%lld, null priv / values", (long long)M);
        return R.critic_values(M, priv, values, shadow);
    });
}

// Test hook, not part of include/hgym.h: out[0..3] = KB, KR, NC, nlast of a first layer (struct L0KSteps) -- cfg == NULL: of input
// width K by l0_ksteps alone; else: as ws_layout lays out net `which` of cfg (K ignored).  Host arithmetic only, no device call.
int32_t hgym_internal_l0_ksteps(const HgymNetConfig* cfg, int32_t which, int32_t K, int32_t* out) {
    HG_REQUIRE(out, HGYM_E_BADARG, "null out");
    L0KSteps s;
    if (cfg) {
        WsLayout w;
        const int32_t rc = ws_layout(cfg, &w);
        if (rc) return rc;
        HG_REQUIRE(which >= 0 && which < w.nnets && w.net[which].fused, HGYM_E_BADARG, "which=%d: not a net on the fused layout", which);
        const LayerLayout& y = w.net[which].layer[0];
        s.KB = y.KBf;
        s.KR = y.KRf;
        s.NC = y.KBf / 4;
        s.nlast = y.KRf - 4 * (s.NC - 1);
    } else {
        HG_REQUIRE(K > 0, HGYM_E_BADARG, "K=%d", K);
        s = l0_ksteps(K);
    }
    out[0] = s.KB;
    out[1] = s.KR;
    out[2] = s.NC;
    out[3] = s.nlast;
    return HGYM_OK;
}

int64_t hgym_net_shadow_ld(const HgymNetConfig* cfg, int32_t which) {
    WsLayout w;
    if (ws_layout(cfg, &w) != HGYM_OK || which < 0 || which > 1 || !w.net[which].fused) return 0;
    return shadow_ld(w, which);
}

int32_t hgym_policy_act(const HgymNetConfig* cfg, const HgymNet* net, int32_t M, const float* obs, const float* priv, const float* z,
                        uint64_t seed, const int64_t* step_counter, float* actions, float* mu, float* sigma, float* logp, float* values,
                        const HgymObsShadow* shadow, void* stream) {
    return run(cfg, net, stream, [&](auto& R) -> int32_t {
        HG_REQUIRE(obs && priv && actions && mu && sigma && logp && values, HGYM_E_BADARG, "null pointer");
        return R.act(M, obs, priv, z, seed, step_counter, actions, mu, sigma, logp, values, nullptr, shadow);
    });
}

int32_t hgym_policy_act_fin(const HgymNetConfig* cfg, const HgymNet* net, int32_t M, const float* obs, const float* priv, const float* z,
                            uint64_t seed, const int64_t* step_counter, float* actions, float* mu, float* sigma, float* logp,
                            float* values, const HgymEnvConfig* env_cfg, const HgymEnvState* env_st, const HgymEnvOut* env_out,
                            const HgymObsShadow* shadow, void* stream) {
    return run(cfg, net, stream, [&](auto& R) -> int32_t {
        HG_REQUIRE(obs && priv && actions && mu && sigma && logp && values, HGYM_E_BADARG, "null pointer");
        HG_REQUIRE(env_cfg && env_st && env_out, HGYM_E_BADARG, "null env cfg/state/out");
        HG_REQUIRE(env_st->counters && env_st->episode_acc && env_out->time_out && env_out->extras_time_outs && env_out->extras_episode &&
                       env_out->rew && env_out->reset, HGYM_E_BADARG, "null finaliser buffer");
        HG_REQUIRE(env_cfg->num_envs > 0, HGYM_E_SHAPE, "num_envs=%d", env_cfg->num_envs);
        const FinArgs fin = make_fin_args(*env_cfg, *env_st, *env_out, FIN_MODE_STEP);
        return R.act(M, obs, priv, z, seed, step_counter, actions, mu, sigma, logp, values, &fin, shadow);
    });
}

// Behind hgym_ppo_grad, hgym_ppo_grad_part, hgym_ppo_grad_smooth, hgym_ppo_grad_smooth_mirror and hgym_ppo_grad_guide: the checks they
// share, in one order, then the actor's head (struct ActorHead) and the runner's grad.  part: null for the whole gradient, else
// hgym_ppo_grad_part's half; smooth, head_partials, guide: what the entry point has of them, else null.
static int32_t ppo_grad_entry(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* batch,
                              const int32_t* part, const HgymSmooth* smooth, float* head_partials, const HgymGuide* guide, void* stream) {
    return run(cfg, net, stream, [&](auto& R) -> int32_t {
        int32_t rc = check_ppo(ppo);
        if (rc) return rc;
        HG_REQUIRE(!part || *part == 0 || *part == 1, HGYM_E_BADARG, "part=%d (0 or 1)", *part);
        HG_REQUIRE(net->grads && net->opt_state, HGYM_E_BADARG, "null grads / opt_state");
        rc = check_batch(R.w, ppo, batch);
        return rc ? rc : R.grad(*ppo, *batch, part ? *part : -1, actor_head(*ppo, batch->B, cfg->num_actions, smooth, head_partials, guide));
    });
}

int32_t hgym_ppo_grad(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* batch, void* stream) {
    return ppo_grad_entry(cfg, ppo, net, batch, nullptr, nullptr, nullptr, nullptr, stream);
}

// What hgym_ppo_grad_smooth and hgym_ppo_grad_smooth_mirror refuse of an HgymSmooth, the same for both (fn: the caller's name)
// alone: hgym_ppo_grad_smooth, which also refuses the mirror loss (at the place in the order it always had)
static int32_t check_smooth(const HgymPPOConfig* ppo, const HgymSmooth* smooth, const char* fn, bool alone) {
    const float lt = smooth->temporal_coef, ls = smooth->spatial_coef;
    // (written so that a NaN fails it)
    HG_REQUIRE(lt >= 0.0f && lt < INFINITY && ls >= 0.0f && ls < INFINITY, HGYM_E_BADARG,
               "HgymSmooth.temporal_coef=%g / spatial_coef=%g must be finite and >= 0 (0: that term is off)", (double)lt, (double)ls);
    HG_REQUIRE(!alone || !(ppo->mirror_coef > 0.0f), HGYM_E_BADARG, "hgym_ppo_grad_smooth with HgymPPOConfig.mirror_coef > 0: the two heads do not combine");
    HG_REQUIRE(ppo->world_size <= 1, HGYM_E_BADARG, "%s with world_size=%d: one rank only", fn, ppo->world_size);
    if (lt > 0.0f || ls > 0.0f) {
        HG_REQUIRE(smooth->sums && ((uintptr_t)smooth->sums & 7) == 0, HGYM_E_BADARG, "HgymSmooth.sums must be non-null and 8-byte aligned");
        if (lt > 0.0f) {
            HG_REQUIRE(smooth->next_idx && smooth->next_weight && smooth->target_next, HGYM_E_BADARG,
                       "HgymSmooth.temporal_coef > 0 needs next_idx, next_weight and target_next");
            HG_REQUIRE(((uintptr_t)smooth->target_next & 15) == 0 && ((uintptr_t)smooth->next_idx & 7) == 0 && ((uintptr_t)smooth->next_weight & 3) == 0,
                       HGYM_E_BADARG, "HgymSmooth.target_next must be 16-byte aligned (next_idx 8, next_weight 4)");
        }
        if (ls > 0.0f) {
            HG_REQUIRE(smooth->noise_std && smooth->target_near && smooth->rows, HGYM_E_BADARG,
                       "HgymSmooth.spatial_coef > 0 needs noise_std, target_near and rows");
            HG_REQUIRE((((uintptr_t)smooth->target_near | (uintptr_t)smooth->rows) & 15) == 0 && ((uintptr_t)smooth->noise_std & 3) == 0, HGYM_E_BADARG,
                       "HgymSmooth.target_near and rows must be 16-byte aligned (noise_std 4)");
        }
    }
    return HGYM_OK;
}

int32_t hgym_ppo_grad_smooth(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* batch,
                             const HgymSmooth* smooth, void* stream) {
    // every refusal below comes before anything is launched
    HG_REQUIRE(cfg && ppo && net && batch && smooth, HGYM_E_BADARG, "hgym_ppo_grad_smooth: null cfg / ppo / net / batch / smooth");
    const int32_t rc = check_smooth(ppo, smooth, "hgym_ppo_grad_smooth", true);
    if (rc) return rc;
    return ppo_grad_entry(cfg, ppo, net, batch, nullptr, smooth, nullptr, nullptr, stream);
}

int32_t hgym_ppo_grad_smooth_mirror(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* batch,
                                    const HgymSmooth* smooth, float* head_partials, int64_t head_partials_len, void* stream) {
    // every refusal below comes before anything is launched
    HG_REQUIRE(cfg && ppo && net && batch && smooth, HGYM_E_BADARG, "hgym_ppo_grad_smooth_mirror: null cfg / ppo / net / batch / smooth");
    const int32_t rc = check_smooth(ppo, smooth, "hgym_ppo_grad_smooth_mirror", false);
    if (rc) return rc;
    const bool all = ppo->mirror_coef > 0.0f && smooth_on(smooth);
    if (all) {      // (else hgym_ppo_grad_smooth or hgym_ppo_grad: head_partials is not looked at)
        HG_REQUIRE(batch->B >= 1, HGYM_E_BADARG, "hgym_ppo_grad_smooth_mirror: B=%d", batch->B);
        const int64_t need = 4 * (((int64_t)batch->B + 63) / 64);
        HG_REQUIRE(head_partials && ((uintptr_t)head_partials & 15) == 0, HGYM_E_BADARG,
                   "hgym_ppo_grad_smooth_mirror: head_partials must be non-null and 16-byte aligned");
        HG_REQUIRE(head_partials_len >= need, HGYM_E_BADARG, "hgym_ppo_grad_smooth_mirror: head_partials_len=%lld, B=%d needs %lld floats",
                   (long long)head_partials_len, batch->B, (long long)need);
    }
    return ppo_grad_entry(cfg, ppo, net, batch, nullptr, smooth, head_partials, nullptr, stream);
}

int32_t hgym_ppo_grad_guide(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* batch,
                            const HgymGuide* guide, void* stream) {
    // every refusal below comes before anything is launched
    HG_REQUIRE(cfg && ppo && net && batch && guide, HGYM_E_BADARG, "hgym_ppo_grad_guide: null cfg / ppo / net / batch / guide");
    HG_REQUIRE(guide->teacher_mu && guide->coef && guide->sums, HGYM_E_BADARG, "hgym_ppo_grad_guide: null HgymGuide.teacher_mu / coef / sums");
    HG_REQUIRE(((uintptr_t)guide->teacher_mu & 15) == 0 && ((uintptr_t)guide->coef & 3) == 0 && ((uintptr_t)guide->sums & 7) == 0, HGYM_E_BADARG,
               "hgym_ppo_grad_guide: HgymGuide.teacher_mu must be 16-byte aligned (coef 4, sums 8)");
    HG_REQUIRE(!(ppo->mirror_coef > 0.0f), HGYM_E_BADARG, "hgym_ppo_grad_guide with HgymPPOConfig.mirror_coef > 0: the two heads do not combine");
    HG_REQUIRE(ppo->world_size <= 1, HGYM_E_BADARG, "hgym_ppo_grad_guide with world_size=%d: one rank only", ppo->world_size);
    return ppo_grad_entry(cfg, ppo, net, batch, nullptr, nullptr, nullptr, guide, stream);
}

int32_t hgym_ppo_grad_part(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, const HgymBatch* batch, int32_t part,
                           void* stream) {
    return ppo_grad_entry(cfg, ppo, net, batch, &part, nullptr, nullptr, nullptr, stream);
}

int32_t hgym_bc_grad(const HgymNetConfig* cfg, const HgymBCConfig* bc, const HgymNet* net, const HgymBatch* batch, const float* target,
                     double* sums, void* stream) {
    // every refusal below comes before anything is launched (and before any pointer of `net` is looked at)
    HG_REQUIRE(cfg && bc && net && batch, HGYM_E_BADARG, "hgym_bc_grad: null cfg / bc / net / batch");
    HG_REQUIRE(target && sums, HGYM_E_BADARG, "hgym_bc_grad: null target / sums");
    HG_REQUIRE(((uintptr_t)sums & 7) == 0 && ((uintptr_t)target & 3) == 0, HGYM_E_BADARG, "hgym_bc_grad: misaligned target / sums");
    HG_REQUIRE(bc->loss_type == HGYM_BC_MSE || bc->loss_type == HGYM_BC_HUBER, HGYM_E_BADARG,
               "HgymBCConfig.loss_type=%d (HGYM_BC_MSE = 0, HGYM_BC_HUBER = 1)", bc->loss_type);
    // (written so that a NaN fails it)
    HG_REQUIRE(bc->loss_type != HGYM_BC_HUBER || (bc->huber_delta > 0.0f && bc->huber_delta < INFINITY), HGYM_E_BADARG,
               "HgymBCConfig.huber_delta=%g must be finite and > 0", (double)bc->huber_delta);
    HG_REQUIRE(batch->B >= 1 && batch->B <= cfg->max_batch, HGYM_E_BADARG, "hgym_bc_grad: B=%d outside [1, max_batch = %d]", batch->B,
               cfg->max_batch);
    HG_REQUIRE(batch->obs && batch->idx, HGYM_E_BADARG, "hgym_bc_grad: null HgymBatch.obs / idx");
    return run(cfg, net, stream, [&](auto& R) -> int32_t {
        HG_REQUIRE(net->grads && net->opt_state, HGYM_E_BADARG, "null grads / opt_state");
        HG_REQUIRE(!net->norm, HGYM_E_UNSUPPORTED, "hgym_bc_grad with HgymNet.norm set: observation normalisation is not part of a cloning step");
        return R.bc_grad(*bc, *batch, target, sums);
    });
}

// What hgym_vf_grad and hgym_bc_vf_grad refuse of the value half, the same for both (fn: the caller's name); before anything is launched
static int32_t check_vf(const HgymNetConfig* cfg, const HgymVFConfig* vf, const HgymBatch* batch, const double* sums, const char* fn) {
    HG_REQUIRE(sums && ((uintptr_t)sums & 7) == 0, HGYM_E_BADARG, "%s: the value loss's sums must be non-null and 8-byte aligned", fn);
    HG_REQUIRE((vf->unclipped == 0 || vf->unclipped == 1) && (vf->keep_others == 0 || vf->keep_others == 1), HGYM_E_BADARG,
               "%s: HgymVFConfig.unclipped=%d, keep_others=%d (0 or 1 each)", fn, vf->unclipped, vf->keep_others);
    // (written so that a NaN fails it)
    HG_REQUIRE(vf->value_coef >= 0.0f && vf->value_coef < INFINITY, HGYM_E_BADARG, "%s: HgymVFConfig.value_coef=%g must be finite and >= 0", fn,
               (double)vf->value_coef);
    HG_REQUIRE(vf->unclipped || (vf->clip_param >= 0.0f && vf->clip_param < INFINITY), HGYM_E_BADARG,
               "%s: HgymVFConfig.clip_param=%g must be finite and >= 0", fn, (double)vf->clip_param);
    HG_REQUIRE(batch->B >= 1 && batch->B <= cfg->max_batch, HGYM_E_BADARG, "%s: B=%d outside [1, max_batch = %d]", fn, batch->B, cfg->max_batch);
    HG_REQUIRE(batch->priv && batch->returns && batch->idx, HGYM_E_BADARG, "%s: null HgymBatch.priv / returns / idx", fn);
    HG_REQUIRE(vf->unclipped || batch->values, HGYM_E_BADARG, "%s: the clipped value loss needs HgymBatch.values", fn);
    HG_REQUIRE((((uintptr_t)batch->priv | (uintptr_t)batch->returns | (uintptr_t)batch->values) & 3) == 0 && ((uintptr_t)batch->idx & 7) == 0 &&
                   ((uintptr_t)batch->priv_bf16 & 15) == 0, HGYM_E_BADARG, "%s: misaligned HgymBatch.priv / returns / values / idx / priv_bf16", fn);
    return HGYM_OK;
}

int32_t hgym_vf_grad(const HgymNetConfig* cfg, const HgymVFConfig* vf, const HgymNet* net, const HgymBatch* batch, double* sums, void* stream) {
    // every refusal below comes before anything is launched (and before any pointer of `net` is looked at)
    HG_REQUIRE(cfg && vf && net && batch, HGYM_E_BADARG, "hgym_vf_grad: null cfg / vf / net / batch");
    const int32_t rc = check_vf(cfg, vf, batch, sums, "hgym_vf_grad");
    if (rc) return rc;
    return run(cfg, net, stream, [&](auto& R) -> int32_t {
        HG_REQUIRE(net->grads && net->opt_state, HGYM_E_BADARG, "null grads / opt_state");
        return R.vf_grad(*vf, *batch, sums);
    });
}

int32_t hgym_bc_vf_grad(const HgymNetConfig* cfg, const HgymBCConfig* bc, const HgymVFConfig* vf, const HgymNet* net, const HgymBatch* batch,
                        const float* target, double* bc_sums, double* vf_sums, void* stream) {
    // every refusal below comes before anything is launched: hgym_bc_grad's, then hgym_vf_grad's
    HG_REQUIRE(cfg && bc && vf && net && batch, HGYM_E_BADARG, "hgym_bc_vf_grad: null cfg / bc / vf / net / batch");
    HG_REQUIRE(target && bc_sums, HGYM_E_BADARG, "hgym_bc_vf_grad: null target / bc_sums");
    HG_REQUIRE(((uintptr_t)bc_sums & 7) == 0 && ((uintptr_t)target & 3) == 0, HGYM_E_BADARG, "hgym_bc_vf_grad: misaligned target / bc_sums");
    HG_REQUIRE(bc->loss_type == HGYM_BC_MSE || bc->loss_type == HGYM_BC_HUBER, HGYM_E_BADARG,
               "HgymBCConfig.loss_type=%d (HGYM_BC_MSE = 0, HGYM_BC_HUBER = 1)", bc->loss_type);
    // (written so that a NaN fails it)
    HG_REQUIRE(bc->loss_type != HGYM_BC_HUBER || (bc->huber_delta > 0.0f && bc->huber_delta < INFINITY), HGYM_E_BADARG,
               "HgymBCConfig.huber_delta=%g must be finite and > 0", (double)bc->huber_delta);
    const int32_t rc = check_vf(cfg, vf, batch, vf_sums, "hgym_bc_vf_grad");
    if (rc) return rc;
    HG_REQUIRE(bc_sums != vf_sums, HGYM_E_BADARG, "hgym_bc_vf_grad: bc_sums and vf_sums must be two blocks");
    HG_REQUIRE(batch->obs && ((uintptr_t)batch->obs_bf16 & 15) == 0, HGYM_E_BADARG, "hgym_bc_vf_grad: null HgymBatch.obs, or a misaligned obs_bf16");
    return run(cfg, net, stream, [&](auto& R) -> int32_t {
        HG_REQUIRE(net->grads && net->opt_state, HGYM_E_BADARG, "null grads / opt_state");
        HG_REQUIRE(!net->norm, HGYM_E_UNSUPPORTED, "hgym_bc_vf_grad with HgymNet.norm set: observation normalisation is not part of a cloning step");
        return R.bc_vf_grad(*bc, *vf, *batch, target, bc_sums, vf_sums);
    });
}

int64_t hgym_net_param_offset(const HgymNetConfig* cfg, int32_t which) {
    WsLayout w;
    if (ws_layout(cfg, &w) != HGYM_OK) return -1;
    if (which < 0 || which >= w.nnets) return which == w.nnets ? w.P : -1;
    return w.net[which].layer[0].w_off;
}

int32_t hgym_ppo_apply(const HgymNetConfig* cfg, const HgymPPOConfig* ppo, const HgymNet* net, void* stream) {
    return run(cfg, net, stream, [&](auto& R) -> int32_t {
        const int32_t rc = check_ppo(ppo);
        if (rc) return rc;
        HG_REQUIRE(net->grads && net->adam_m && net->adam_v && net->opt_state, HGYM_E_BADARG, "null optimiser buffers");
        return R.apply(*ppo);
    });
}

}  // extern "C"
