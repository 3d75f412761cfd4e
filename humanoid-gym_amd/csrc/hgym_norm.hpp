// hgym_norm.hpp -- layout of the observation normaliser's block (HgymNet.norm) and what hgym_net.hip and hgym_norm.hip ask of each other.
#pragma once
#include "hgym_common.hpp"

namespace hgym {

constexpr int NORM_ROWS_PER_WG = 64;    // rows of one row block of norm_accumulate_kernel (16 groups of four rows)
constexpr int NORM_WGS = 512;           // its workgroups, dealt to the two row kinds by their row length
constexpr int NORM_THREADS = 768;
constexpr int NORM_HEADER_DOUBLES = 8;  // eps, until, count[2], rest unused

// Byte offsets inside the block (256-byte aligned parts); stat 0 = the actor's columns (num_obs, shared by the auxiliary head), 1 = the critic's.
struct NormLayout {
    int K[2];              // columns per stat
    int N1[3];             // first-layer outputs of actor, critic, auxiliary head (0: absent)
    int wgs[2];            // workgroups of the accumulate launch per row kind (= rows of its partial sums)
    int64_t header;        // [NORM_HEADER_DOUBLES] fp64
    int64_t mean[2], var[2];       // fp64 [K]
    int64_t mf[2], sf[2];          // fp32 [K]: (float)mean, (float)(1 / (sqrt(var) + eps))
    int64_t eb[3];                 // fp32 [N1]: the effective first-layer bias of each net (-1: absent)
    int64_t sums;                  // fp64: [n | sum x [K0] | sum x^2 [K0] | n | sum x [K1] | sum x^2 [K1]]
    int64_t sums_doubles;
    int64_t partials[2];           // fp64 [wgs][2][K]
    int64_t bytes;
};

// From the widths alone (the caller has validated the configuration: net_first_layers).
static inline void norm_layout(const HgymNetConfig* c, NormLayout* n) {
    memset(n, 0, sizeof(*n));
    n->K[0] = c->num_obs;
    n->K[1] = c->num_priv;
    n->N1[0] = c->actor_dims[1];
    n->N1[1] = c->critic_dims[1];
    n->N1[2] = c->aux_layers > 0 ? c->aux_dims[1] : 0;
    const int64_t kk = (int64_t)n->K[0] + n->K[1];
    n->wgs[0] = (int)((int64_t)NORM_WGS * n->K[0] / kk);
    if (n->wgs[0] < 1) n->wgs[0] = 1;
    if (n->wgs[0] > NORM_WGS - 1) n->wgs[0] = NORM_WGS - 1;
    n->wgs[1] = NORM_WGS - n->wgs[0];
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        const int64_t o = off;
        off += round_up(bytes, 256);
        return o;
    };
    n->header = take(NORM_HEADER_DOUBLES * 8);
    for (int s = 0; s < 2; ++s) {
        n->mean[s] = take((int64_t)n->K[s] * 8);
        n->var[s] = take((int64_t)n->K[s] * 8);
    }
    for (int s = 0; s < 2; ++s) {
        n->mf[s] = take((int64_t)n->K[s] * 4);
        n->sf[s] = take((int64_t)n->K[s] * 4);
    }
    for (int i = 0; i < 3; ++i) n->eb[i] = n->N1[i] > 0 ? take((int64_t)n->N1[i] * 4) : -1;
    n->sums_doubles = 2 + 2 * kk;
    n->sums = take(n->sums_doubles * 8);
    for (int s = 0; s < 2; ++s) n->partials[s] = take((int64_t)n->wgs[s] * 2 * n->K[s] * 8);
    n->bytes = off;
}

// first layer of net i in the flat parameter vector
struct NormFirst {
    int64_t w_off, b_off;
    int N, K;
};

// hgym_net.hip
int32_t net_first_layers(const HgymNetConfig* cfg, NormFirst out[3], int* nnets);       // validates cfg (ws_layout)
int32_t net_norm_refold(const HgymNetConfig* cfg, const HgymNet* net, void* stream);    // first-layer operand copies, then norm_fold_bias
// hgym_norm.hip: effective biases of every net from the master parameters and the derived floats
int32_t norm_fold_bias(const HgymNetConfig* cfg, const HgymNet* net, hipStream_t s);

}  // namespace hgym
