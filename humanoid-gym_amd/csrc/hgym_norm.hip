// hgym_norm.hip -- empirical observation normalisation folded into the first layer: running per-column statistics in
// fp64 (rsl_rl's EmpiricalNormalization merge), their float forms, the effective first-layer biases, and the gradient unfold.  No kernel of the
// forward or the update reads anything here but the effective bias and the scaled operand copies that hgym_net.hip writes.
// Built with -ffp-contract=off: tests/obs_norm_common.py restates every expression with one rounding per operation.
#include "hgym_norm.hpp"

namespace hgym {

constexpr int NORM_MAX_WIDTH = 1024;     // LDS of norm_accumulate_kernel: 80 bytes per column above 384 columns

// ------------------------------------------------------------------------------------------------ accumulate
struct NormAccArgs {
    const float* x[2];     // (M, K) row-major, contiguous
    int K[2];
    int vec[2];            // the 16-byte path: x is 16-byte aligned
    int wgs[2];            // workgroups of this launch per kind (blockIdx.x < wgs[0]: kind 0)
    int64_t M;
    double* part[2];       // [wgs][2][K]
};

// Column sums and sums of squares of M rows, fp64, as per-workgroup partials.
// Rows are K floats long and only 4-byte aligned (705 floats = 2820 bytes), but FOUR rows are 16 K bytes: lane t of a group always reads the 16
// bytes at element 4 t of a four-row group, whose four elements are then the same four (row phase, column) pairs in every group -- (4 t + e) / K,
// (4 t + e) % K -- so a lane keeps eight fp64 accumulators in registers, every load is a 16-byte one, and a wavefront reads 1 KiB contiguously.
// K <= 384: floor(768 / K) four-row groups side by side.  Workgroup b walks the 64-row blocks b, b + wgs, ... (a static deal: the partial of a
// workgroup is a fixed sequence of additions); the phases, the side-by-side groups and the up-to-three leftover rows of the last block (4-byte
// loads) meet in LDS and are added per column in slot order.  No atomics anywhere: the same rows give the same bits.
__global__ __launch_bounds__(NORM_THREADS) void norm_accumulate_kernel(const NormAccArgs a) {
    extern __shared__ double lds[];      // [slots][2][K], slots = 4 G + 1
    const int kind = (int)blockIdx.x < a.wgs[0] ? 0 : 1;
    const int wg = kind ? (int)blockIdx.x - a.wgs[0] : (int)blockIdx.x;
    const int nwg = a.wgs[kind];
    const int K = a.K[kind];
    const float* __restrict__ x = a.x[kind];
    const int64_t M = a.M;
    const int64_t nblk = (M + NORM_ROWS_PER_WG - 1) / NORM_ROWS_PER_WG;
    const bool vec = a.vec[kind] != 0;
    int G = K <= NORM_THREADS / 2 ? NORM_THREADS / K : 1;
    if (G > NORM_ROWS_PER_WG / 4) G = NORM_ROWS_PER_WG / 4;
    const int tid = threadIdx.x;
    if (vec) {
        const int span = G * K;      // G > 1: one pass (G K <= 768); G = 1: the lanes walk the K positions in passes of 768
        for (int q = tid; q < span; q += NORM_THREADS) {
            const int g = q / K, t = q - g * K;
            double sx[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
            for (int64_t rb = wg; rb < nblk; rb += nwg) {
                const int64_t r0 = rb * NORM_ROWS_PER_WG;
                const int rows = (int)(M - r0 < NORM_ROWS_PER_WG ? M - r0 : NORM_ROWS_PER_WG);
                const int ngr = rows >> 2;
                const float* p = x + r0 * K + 4 * (int64_t)t;
#pragma unroll 4
                for (int sr = g; sr < ngr; sr += G) {
                    const float4 v = *reinterpret_cast<const float4*>(p + (int64_t)sr * 4 * K);
                    const double d0 = (double)v.x, d1 = (double)v.y, d2 = (double)v.z, d3 = (double)v.w;
                    sx[0] += d0; sq[0] += d0 * d0;
                    sx[1] += d1; sq[1] += d1 * d1;
                    sx[2] += d2; sq[2] += d2 * d2;
                    sx[3] += d3; sq[3] += d3 * d3;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 4 * t + e, r = i / K, c = i - r * K;
                lds[((int64_t)(g * 4 + r) * 2 + 0) * K + c] = sx[e];
                lds[((int64_t)(g * 4 + r) * 2 + 1) * K + c] = sq[e];
            }
        }
    } else {
        for (int i = tid; i < 4 * G * 2 * K; i += NORM_THREADS) lds[i] = 0.0;
    }
    // what the 16-byte path leaves: the last block's rows beyond a multiple of four -- or, for rows that are not 16-byte aligned, every row
    for (int c = tid; c < K; c += NORM_THREADS) {
        double sx = 0.0, sq = 0.0;
        for (int64_t rb = wg; rb < nblk; rb += nwg) {
            const int64_t r0 = rb * NORM_ROWS_PER_WG;
            const int rows = (int)(M - r0 < NORM_ROWS_PER_WG ? M - r0 : NORM_ROWS_PER_WG);
            for (int r = vec ? (rows & ~3) : 0; r < rows; ++r) {
                const double d = (double)x[(r0 + r) * K + c];
                sx += d;
                sq += d * d;
            }
        }
        lds[((int64_t)(4 * G) * 2 + 0) * K + c] = sx;
        lds[((int64_t)(4 * G) * 2 + 1) * K + c] = sq;
    }
    __syncthreads();
    double* __restrict__ out = a.part[kind] + (int64_t)wg * 2 * K;
    for (int i = tid; i < 2 * K; i += NORM_THREADS) {
        const int j = i / K, c = i - j * K;
        double s = 0.0;
        for (int sl = 0; sl <= 4 * G; ++sl) s += lds[((int64_t)sl * 2 + j) * K + c];
        out[i] = s;
    }
}

// sums[kind] = [n | sum x | sum x^2]: the partials of the launch above added in workgroup order
__global__ __launch_bounds__(256) void norm_sums_kernel(int K0, int K1, int w0, int w1, int64_t M, const double* __restrict__ p0,
                                                        const double* __restrict__ p1, double* __restrict__ sums) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n0 = 2 * K0, n1 = 2 * K1;
    if (i >= n0 + n1) return;
    const int kind = i < n0 ? 0 : 1;
    const int j = kind ? i - n0 : i, n = kind ? n1 : n0, w = kind ? w1 : w0;
    const double* p = kind ? p1 : p0;
    double s = 0.0;
    for (int b = 0; b < w; ++b) s += p[(int64_t)b * n + j];
    double* out = sums + (kind ? 1 + n0 : 0);
    out[1 + j] = s;
    if (j == 0) out[0] = (double)M;
}

// ------------------------------------------------------------------------------------------------ init, merge
struct NormStat {
    double* mean;
    double* var;
    float* mf;
    float* sf;
    const double* sums;      // [n | sum x | sum x^2], null for init
    int K;
};

__device__ __forceinline__ void norm_derive(const NormStat& s, int c, double mean, double var, double eps) {
    s.mf[c] = (float)mean;
    s.sf[c] = (float)(1.0 / (sqrt(var) + eps));
}

__global__ __launch_bounds__(1024) void norm_init_kernel(NormStat s0, NormStat s1, double* __restrict__ hdr, double* __restrict__ sums,
                                                         int64_t sums_doubles, double eps, double until) {
    for (int k = 0; k < 2; ++k) {
        const NormStat& s = k ? s1 : s0;
        for (int c = threadIdx.x; c < s.K; c += blockDim.x) {
            s.mean[c] = 0.0;
            s.var[c] = 1.0;
            norm_derive(s, c, 0.0, 1.0, eps);
        }
    }
    for (int64_t i = threadIdx.x; i < sums_doubles; i += blockDim.x) sums[i] = 0.0;
    if (threadIdx.x < NORM_HEADER_DOUBLES) hdr[threadIdx.x] = threadIdx.x == 0 ? eps : (threadIdx.x == 1 ? until : 0.0);
}

// rsl_rl's EmpiricalNormalization.update from the batch's raw sums, per column, fp64; one workgroup (924 columns for XBot-L), so that the
// counts -- which every column reads -- move behind a barrier.  A stat whose count has reached `until`, or whose batch is empty, stays (its
// floats are derived again from the state as it stands).
__global__ __launch_bounds__(1024) void norm_merge_kernel(NormStat s0, NormStat s1, double* __restrict__ hdr) {
    const double eps = hdr[0], until = hdr[1];
    double cnt_new[2];
    for (int k = 0; k < 2; ++k) {
        const NormStat& s = k ? s1 : s0;
        const double count = hdr[2 + k], n = s.sums[0];
        const bool skip = !(n > 0.0) || (until >= 0.0 && count >= until);
        cnt_new[k] = skip ? count : count + n;
        if (skip) {      // the floats all the same: a loaded state (the caller wrote mean / var, cleared the sums) gets them here
            for (int c = threadIdx.x; c < s.K; c += blockDim.x) norm_derive(s, c, s.mean[c], s.var[c], eps);
            continue;
        }
        const double rate = n / cnt_new[k];
        for (int c = threadIdx.x; c < s.K; c += blockDim.x) {
            const double mu_b = s.sums[1 + c] / n;
            double var_b = s.sums[1 + s.K + c] / n - mu_b * mu_b;
            if (!(var_b > 0.0)) var_b = 0.0;
            const double mean = s.mean[c], var = s.var[c];
            const double d = mu_b - mean;
            const double mean_new = mean + rate * d;
            double var_new = var + rate * (var_b - var + d * (mu_b - mean_new));
            if (!(var_new > 0.0)) var_new = 0.0;
            s.mean[c] = mean_new;
            s.var[c] = var_new;
            norm_derive(s, c, mean_new, var_new, eps);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2) hdr[2 + threadIdx.x] = cnt_new[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ fold, unfold
struct NormNetArgs {
    int nnets;
    NormFirst f[3];
    const float* mf[3];
    const float* sf[3];
    float* eb[3];
};

// b'[r] = b[r] - sum_c Wop[r][c] m[c], Wop = T(w s[c]) as the operand copies hold it.  One wavefront per row: lane l adds columns l, l + 64, ...
// in fp64, the 64 lane sums meet in a fixed tree, one rounding to fp32 at the end.
template <typename T>
__global__ __launch_bounds__(256) void norm_fold_kernel(const NormNetArgs a, const float* __restrict__ params) {
    const int net = blockIdx.y;
    const NormFirst f = a.f[net];
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= f.N) return;
    const float* __restrict__ w = params + f.w_off + (int64_t)r * f.K;
    const float* __restrict__ m = a.mf[net];
    const float* __restrict__ s = a.sf[net];
    double acc = 0.0;
    for (int c = lane; c < f.K; c += 64) {
        const float ws = w[c] * s[c];
        const T wt = (T)ws;
        acc += (double)(float)wt * (double)m[c];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) a.eb[net][r] = (float)((double)params[f.b_off + r] - acc);
}

// Gradients of the operand parametrisation (W s, b - W s m) -> of the master one, in place: G_W = (G'_W - g_b m) s, g_b unchanged.
__global__ __launch_bounds__(256) void norm_unfold_kernel(const NormNetArgs a, float* __restrict__ grads) {
    const int net = blockIdx.y;
    const NormFirst f = a.f[net];
    const int64_t n = (int64_t)f.N * f.K;
    const float* __restrict__ m = a.mf[net];
    const float* __restrict__ s = a.sf[net];
    float* __restrict__ gw = grads + f.w_off;
    const float* __restrict__ gb = grads + f.b_off;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / f.K), c = (int)(i - (int64_t)r * f.K);
        const float p = gb[r] * m[c];
        const float d = gw[i] - p;
        gw[i] = d * s[c];
    }
}

struct NormCtx {
    NormLayout l;
    NormNetArgs nets;
    char* base;
    template <typename U> U* at(int64_t off) const { return reinterpret_cast<U*>(base + off); }
    NormStat stat(int k, bool with_sums) const {
        const double* sums = at<double>(l.sums) + (k ? 1 + 2 * l.K[0] : 0);
        return NormStat{at<double>(l.mean[k]), at<double>(l.var[k]), at<float>(l.mf[k]), at<float>(l.sf[k]), with_sums ? sums : nullptr, l.K[k]};
    }
};

static int32_t norm_ctx(const HgymNetConfig* cfg, const HgymNet* net, NormCtx* x) {
    HG_REQUIRE(cfg && net, HGYM_E_BADARG, "null net config / net");
    memset(x, 0, sizeof(*x));
    const int32_t rc = net_first_layers(cfg, x->nets.f, &x->nets.nnets);
    if (rc) return rc;
    HG_REQUIRE(net->norm, HGYM_E_BADARG, "HgymNet.norm is null: this net was set up without observation normalisation");
    HG_REQUIRE(((uintptr_t)net->norm & 255) == 0, HGYM_E_BADARG, "HgymNet.norm must be 256-byte aligned");
    norm_layout(cfg, &x->l);
    x->base = (char*)net->norm;
    for (int i = 0; i < x->nets.nnets; ++i) {
        const int k = i == 1 ? 1 : 0;      // the auxiliary head reads the actor's rows: the actor's statistics
        x->nets.mf[i] = x->at<float>(x->l.mf[k]);
        x->nets.sf[i] = x->at<float>(x->l.sf[k]);
        x->nets.eb[i] = x->at<float>(x->l.eb[i]);
    }
    return HGYM_OK;
}

int32_t norm_fold_bias(const HgymNetConfig* cfg, const HgymNet* net, hipStream_t s) {
    NormCtx x;
    const int32_t rc = norm_ctx(cfg, net, &x);
    if (rc) return rc;
    int rows = 0;
    for (int i = 0; i < x.nets.nnets; ++i) rows = x.nets.f[i].N > rows ? x.nets.f[i].N : rows;
    const dim3 grid(ceil_div(rows, 4), x.nets.nnets);
    if (cfg->precision == HGYM_F32) hipLaunchKernelGGL((norm_fold_kernel<float>), grid, dim3(256), 0, s, x.nets, net->params);
    else hipLaunchKernelGGL((norm_fold_kernel<__bf16>), grid, dim3(256), 0, s, x.nets, net->params);
    HG_CHECK_LAUNCH("norm_fold_kernel");
    return HGYM_OK;
}

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_net_norm_layout(const HgymNetConfig* cfg, int64_t* layout) {
    HG_REQUIRE(cfg && layout, HGYM_E_BADARG, "null net config / layout");
    NormFirst f[3];
    int nnets = 0;
    const int32_t rc = net_first_layers(cfg, f, &nnets);
    if (rc) return rc;
    HG_REQUIRE(cfg->num_obs <= NORM_MAX_WIDTH && cfg->num_priv <= NORM_MAX_WIDTH, HGYM_E_UNSUPPORTED,
               "observation normalisation: rows of %d / %d columns (the accumulate kernel takes up to %d)", cfg->num_obs, cfg->num_priv, NORM_MAX_WIDTH);
    NormLayout l;
    norm_layout(cfg, &l);
    for (int i = 0; i < HGYM_NORM_LAYOUT; ++i) layout[i] = 0;
    layout[HGYM_NORM_BYTES] = l.bytes;
    layout[HGYM_NORM_HEADER] = l.header;
    for (int k = 0; k < 2; ++k) {
        layout[HGYM_NORM_MEAN + k] = l.mean[k];
        layout[HGYM_NORM_VAR + k] = l.var[k];
        layout[HGYM_NORM_MEAN_F + k] = l.mf[k];
        layout[HGYM_NORM_SCALE_F + k] = l.sf[k];
        layout[HGYM_NORM_PARTIALS + k] = l.partials[k];
        layout[HGYM_NORM_WGS + k] = l.wgs[k];
    }
    for (int i = 0; i < 3; ++i) layout[HGYM_NORM_BIAS + i] = l.eb[i];
    layout[HGYM_NORM_SUMS] = l.sums;
    layout[HGYM_NORM_SUMS_DOUBLES] = l.sums_doubles;
    layout[HGYM_NORM_ROWS_PER_WG] = NORM_ROWS_PER_WG;
    return HGYM_OK;
}

int32_t hgym_net_norm_init(const HgymNetConfig* cfg, const HgymNet* net, float eps, int64_t until, void* stream) {
    NormCtx x;
    const int32_t rc = norm_ctx(cfg, net, &x);
    if (rc) return rc;
    HG_REQUIRE(eps >= 0.0f && eps < INFINITY, HGYM_E_BADARG, "observation normalisation: eps=%g must be finite and >= 0", eps);
    HG_REQUIRE(until >= -1, HGYM_E_BADARG, "observation normalisation: until=%lld (-1: never stop, else a row count >= 0)", (long long)until);
    hipLaunchKernelGGL(norm_init_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, x.stat(0, false), x.stat(1, false), x.at<double>(x.l.header),
                       x.at<double>(x.l.sums), x.l.sums_doubles, (double)eps, (double)until);
    HG_CHECK_LAUNCH("norm_init_kernel");
    return HGYM_OK;
}

int32_t hgym_net_norm_accumulate(const HgymNetConfig* cfg, const HgymNet* net, const float* obs, const float* priv, int64_t M, void* stream) {
    NormCtx x;
    const int32_t rc = norm_ctx(cfg, net, &x);
    if (rc) return rc;
    HG_REQUIRE(obs && priv && M > 0, HGYM_E_BADARG, "observation normalisation: null rows / M=%lld", (long long)M);
    HG_REQUIRE(((uintptr_t)obs & 3) == 0 && ((uintptr_t)priv & 3) == 0, HGYM_E_BADARG, "observation rows must be 4-byte aligned");
    HG_REQUIRE(x.l.K[0] <= NORM_MAX_WIDTH && x.l.K[1] <= NORM_MAX_WIDTH, HGYM_E_UNSUPPORTED, "observation normalisation: rows wider than %d columns",
               NORM_MAX_WIDTH);
    HG_REQUIRE(M < ((int64_t)1 << 40), HGYM_E_UNSUPPORTED, "observation normalisation: M=%lld rows", (long long)M);
    NormAccArgs a;
    memset(&a, 0, sizeof(a));
    const int64_t nblk = (M + NORM_ROWS_PER_WG - 1) / NORM_ROWS_PER_WG;
    size_t lds = 0;
    for (int k = 0; k < 2; ++k) {
        a.x[k] = k ? priv : obs;
        a.K[k] = x.l.K[k];
        a.vec[k] = ((uintptr_t)a.x[k] & 15) == 0 ? 1 : 0;
        a.wgs[k] = (int)(nblk < x.l.wgs[k] ? nblk : x.l.wgs[k]);
        a.part[k] = x.at<double>(x.l.partials[k]);
        int G = a.K[k] <= NORM_THREADS / 2 ? NORM_THREADS / a.K[k] : 1;
        if (G > NORM_ROWS_PER_WG / 4) G = NORM_ROWS_PER_WG / 4;
        const size_t need = (size_t)(4 * G + 1) * 2 * a.K[k] * 8;
        lds = need > lds ? need : lds;
    }
    a.M = M;
    const int32_t rc_lds = ensure_dynamic_lds(reinterpret_cast<const void*>(&norm_accumulate_kernel), lds, "norm_accumulate_kernel");
    if (rc_lds) return rc_lds;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(norm_accumulate_kernel, dim3(a.wgs[0] + a.wgs[1]), dim3(NORM_THREADS), lds, s, a);
    HG_CHECK_LAUNCH("norm_accumulate_kernel");
    hipLaunchKernelGGL(norm_sums_kernel, dim3(ceil_div(2 * (a.K[0] + a.K[1]), 256)), dim3(256), 0, s, a.K[0], a.K[1], a.wgs[0], a.wgs[1], M, a.part[0],
                       a.part[1], x.at<double>(x.l.sums));
    HG_CHECK_LAUNCH("norm_sums_kernel");
    return HGYM_OK;
}

int32_t hgym_net_norm_merge(const HgymNetConfig* cfg, const HgymNet* net, void* stream) {
    NormCtx x;
    const int32_t rc = norm_ctx(cfg, net, &x);
    if (rc) return rc;
    hipLaunchKernelGGL(norm_merge_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, x.stat(0, true), x.stat(1, true), x.at<double>(x.l.header));
    HG_CHECK_LAUNCH("norm_merge_kernel");
    return net_norm_refold(cfg, net, stream);
}

int32_t hgym_net_norm_unfold_grad(const HgymNetConfig* cfg, const HgymNet* net, void* stream) {
    NormCtx x;
    const int32_t rc = norm_ctx(cfg, net, &x);
    if (rc) return rc;
    HG_REQUIRE(net->grads, HGYM_E_BADARG, "null grads");
    hipLaunchKernelGGL(norm_unfold_kernel, dim3(256, x.nets.nnets), dim3(256), 0, (hipStream_t)stream, x.nets, net->grads);
    HG_CHECK_LAUNCH("norm_unfold_kernel");
    return HGYM_OK;
}

}  // extern "C"
