// hgym_rollout.hpp -- rollout_step_kernel and its argument records, shared by the translation units that instantiate it: hgym_rollout.hip
// (ELU(1), and the host side of the launch) and hgym_rollout_act.hip (any resolved activation: HgymNetConfig.fused_activation).  Both are built
// with -ffp-contract=off and define HGYM_TU_CONTRACT_OFF before including this file; the design is described at the top of hgym_rollout.hip.
#pragma once
#include <stdlib.h>

#include <algorithm>

#include "hgym_env_math.hpp"
#include "hgym_fused.hpp"


namespace hgym {

int32_t rollout_fwd_args(const HgymNetConfig* cfg, const HgymNet* net, int M, const float* obs, const float* priv, uint64_t seed,
                         const int64_t* step, float* actions, float* mu, float* sigma, float* logp, float* values, FwdArgs* out,
                         size_t* lds_bytes, const HgymObsShadow* sh, const float* z = nullptr);      // z: this step's (M, A) normals in place of the launch's own draw (FwdArgs.z)
int32_t rollout_eval_fwd_args(const HgymNetConfig* cfg, const HgymNet* net, int M, const float* obs, float* actions, FwdArgs* out,
                              size_t* lds_bytes);
int32_t rollout_env_args(const HgymEnvConfig* cfg, const HgymSimTensors* sim, const HgymEnvState* st, const HgymEnvOut* out,
                         float* actions, EnvArgs* A, bool sink = true);

constexpr int RO_E = 32;       // envs (= policy rows) per workgroup
constexpr int RO_NT = 512;     // lanes per workgroup: 8 wavefronts, as mlp_fwd_kernel<32, 8, 4>

// caller's scratch block (HGYM_ROLLOUT_SCRATCH_BYTES(num_envs), zero-filled once): this header, then two per-parity images of the
// env step's draw tables ([tile][125 floats x 32 envs], the layout of the LDS noise tables u_delay .. phys)
struct RolloutScratch {
    int64_t pp[2][4];          // [parity]{common step counter, ring step, sampling step, -}
    int64_t reset_cnt[2];      // [parity] envs that reset in the step of that parity
    int64_t pad[6];
    float acc[2][24];          // [parity] episode-sum accumulators of that step (HgymEnvState::episode_acc layout)
};
static_assert(sizeof(RolloutScratch) <= HGYM_ROLLOUT_SCRATCH_HEADER_BYTES, "scratch block too small");

// The three argument records are SEPARATE kernel parameters: as members of one 3 KB struct the compiler, past some size of the
// kernel body, stopped seeing that the argument block is only read and kept a private-memory copy of all of it.
struct RolloutPP {
    const int64_t* in;         // {common step counter, ring step, sampling step} this launch works with
    int64_t* out;              // the same + 1, written by workgroup (0, 0) for the next launch
    int env_lds_off;           // byte offset of the env image in dynamic LDS (behind the policy tile's buffers)
    // The env step's Philox draws depend on (seed, step, env) only, so the draws of step t + 1 are computed during step t by the
    // CRITIC workgroup of the same tile -- idle for the second half of the launch -- and handed over through global memory:
    // draws_out = where this launch leaves the tables of the next step, draws_in = the tables of this step (null: the first step
    // of a rollout, the actor workgroup computes them itself on its idle wavefronts).  Layout: tile-major, each tile the
    // contiguous LDS noise-table region [u_delay .. phys] of lds_map(32).
    const float* draws_in;
    float* draws_out;
    int draws_len;             // floats per tile
    // The actor's first layer carried across launches (hgym_fused.hpp: L0Part / L0Ahead): l0.acc = what the previous launch's critic
    // workgroups left for this step (PART instantiation), ah.acc_out = where this launch's leave the next step's (null: not).
    L0Part l0;
    L0Ahead ah;
    const uint8_t* prev_reset;   // reset flags of the previous step (prev_out->reset; null: first step of a rollout), see the rows-after-next note below
};

constexpr int RO_NIO = hist_ni<15, HGYM_OBS_FRAME, RO_E, RO_NT>();
constexpr int RO_NIP = hist_ni<3, HGYM_PRIV_FRAME, RO_E, RO_NT>();
// The rows after next (obs_ahead / priv_ahead: 13 + 1 older frames per env, ring -> rows, 78 KB per tile) are copied by the tile's CRITIC
// workgroup at its start, not by the idle wavefronts of the actor workgroup's per-env phase -- in a run of launches that phase waited
// 7 us for the copy's loads and acknowledged stores, against 4.5 us for its own arithmetic, and the critic workgroup ends ~3 us before
// the actor's.  The copy reads pre-reset history for an env that resets in THIS step; nobody reads those rows before the next launch,
// which zeroes them (prev_reset) -- the kernel boundary orders the two workgroups' stores to the same addresses.  (Measured and dropped:
// the copy on the actor workgroup's idle wavefronts, its stores as the launch's last instructions, LDS-only barriers around the per-env
// phase -- profiles/r04_rollout_env_part_findings.txt.)
// The staging phases (env_stage_in / env_stage_out) are instantiated for the one layout this launch accepts (rollout_env_args refuses
// every other): their general paths are compiled out -- 122 -> 108 KB of code, collection 2.99 -> 2.96 ms in a same-call A/B
// (profiles/r05a_bench_ab_base_rofast_dw32.txt).
constexpr int RO_NIA_C = hist_ni<15, HGYM_OBS_FRAME, RO_E, RO_NT, 2>();
constexpr int RO_NIAP_C = hist_ni<3, HGYM_PRIV_FRAME, RO_E, RO_NT, 2>();
constexpr int RO_NIA64 = hist_ni<15, HGYM_OBS_FRAME, 2 * RO_E, RO_NT, 2>();
constexpr int RO_NIAP64 = hist_ni<3, HGYM_PRIV_FRAME, 2 * RO_E, RO_NT, 2>();
constexpr int RO_CHAIN = 64 * kChainRoles;     // lanes of the per-env chain: four wavefronts by role (env_step_phase_a3)

// PRE (HgymEnvOut.obs_older_ready): the 14 older frames of this launch's stacked observation rows were written by the previous launch
// (as its obs_ahead), so the copy ring -> rows -- 11 HBM loads per lane issued after the first layer, in front of the second layer's
// weight ring in the in-order vmcnt queue, and their stores: 4.4 us of a 42 us launch -- is not in this kernel at all.  A launch
// that is given obs_ahead writes the 13 frames it already knows of the rows after next on the seven wavefronts that idle during
// the per-env phase, and this step's frame next to its own row's in the stack phase.
// NOCRITIC (hgym_rollout_step with values = NULL, header v7): no critic tiles -- grid rows = the actor + env workgroups and the
// finaliser; the critic runs once over the stored rows after the rollout (hgym_critic_values).  With PRE = PART = false the actor
// workgroup draws its own random numbers and copies its own history rows, as in the first launch of a rollout.
// C64: the non-actor workgroups in the 64-row layout (see below), instantiated for the steady-state launch (PART) only -- one code
// object for both layouts of every form would exceed the kernel size guard (build.py), and the other forms run once per rollout.
// EVAL (hgym_rollout_eval_step): the NOCRITIC form that just RUNS the policy -- action = mu.  The tile is launched without the sampling
// epilogue (FwdArgs.sample = 0: no Philox draw for the policy, no sigma, no log-probability; the head's outputs go to `actions` through
// FusedNet.out) and hands its head outputs to the env image through fwd_body's head hook instead of the sampling epilogue's put hook.
// A template parameter, so that the training instantiations stay as they were.
// GA: the policy tiles' activation (hgym_fused.hpp) -- false: ELU(1), rollout_step_kernel; true: FwdArgs::act, rollout_step_act_kernel
// (hgym_rollout_act.hip).  The body is one inlined function, so that the ELU(1) kernels keep their names and their code.
template <bool FIN, bool PRE, bool PART, bool NOCRITIC, bool C64, bool EVAL, bool GA>
__device__ __forceinline__ void rollout_step_body(const FwdArgs& f, const EnvArgs& e, const FinArgs& fin, const RolloutPP& pp) {
    static_assert(!NOCRITIC || (!PRE && !PART), "rows ahead and the carried first layer are the critic workgroups' side jobs");
    static_assert(!EVAL || NOCRITIC, "the evaluation launch has no critic tiles");
    static_assert(!C64 || (PRE && PART), "the 64-row layout is instantiated for the steady-state launch");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (FIN && blockIdx.y >= (NOCRITIC ? 1 : 2)) {
        // (phase clock: slot 6 of the env row = when this workgroup of the third grid row started, slot 7 of block 0 = the finaliser's end)
        long long* d2 = f.dbg ? f.dbg + ((int64_t)2 * gridDim.x + blockIdx.x) * 8 : nullptr;
        if (d2 && threadIdx.x == 0) d2[6] = (long long)__builtin_amdgcn_s_memrealtime();
        if (blockIdx.x == 0) {
            fin_block(fin, threadIdx.x, RO_NT);
            if (d2 && threadIdx.x == 0) d2[7] = (long long)__builtin_amdgcn_s_memrealtime();
        }
        return;
    }
    constexpr int U = 16 / 8;                       // n-blocks per wave per 256 first-layer columns (mlp_fwd_kernel)
    // actor and critic workgroups alternate in dispatch order (tile b: row 0 holds its actor when b is even, its critic when b
    // is odd), so that the long actor + env workgroups are spread evenly over neighbouring compute units
    const bool critic_wg = !NOCRITIC && ((blockIdx.x + blockIdx.y) & 1) != 0;
    if constexpr (C64) if (critic_wg) {
        // 64-row layout: the non-actor workgroup of grid column x serves the 64 rows of tiles 2 (x / 2) and
        // 2 (x / 2) + 1, as their CRITIC tile or as their SIDE-JOB workgroup.  A tile's time is its weight stream, not its rows, so
        // one 64-row critic tile costs about what a 32-row one did, and the side jobs get a workgroup of their own.  Of the two
        // columns of a pair one is the critic and one the side job, and the choice flips every 8 columns, so that each XCD (column
        // x mod 8 in both grid rows) receives as many of each role as of the other.
        const int b = (int)blockIdx.x >> 1;
        const bool side = (((int)blockIdx.x ^ ((int)blockIdx.x >> 3)) & 1) != 0;
        // side jobs of rows [64 b, 64 b + 64), in the order the critic workgroup of the 32-row layout runs them: the rows after next
        // (loads issued first, they travel while the draws are computed), the next step's draws, the copy's stores, then the actor's
        // first layer ahead, under whose weight loads the stores are acknowledged.  The critic workgroup, shorter by the first
        // layer ahead, computes the draws of the first of the two tiles behind its own tile, the side-job workgroup those of the second.
        float ha[RO_NIA64][4], hp[RO_NIAP64][4];
        const int ring_s = (int)pp.in[1];
        if (!side) {
            fwd_body<2 * RO_E, 8, 2, 3 * U, false, false, false, GA>(f, f.net[1], false, smem, FwdNoop(), FwdNoop(), FwdNoop(), 0, FwdNoop(), FwdNoop(), nullptr,
                                            nullptr, FwdNoop(), nullptr, b);
        } else {
            phase_stamp(f.dbg, 0);
            hist_load<15, HGYM_OBS_FRAME, RO_NIA64, 2>(e.st.obs_ring, b * 2 * RO_E, 2 * RO_E, ring_s % 15, (int)threadIdx.x, RO_NT, ha);
            hist_load<3, HGYM_PRIV_FRAME, RO_NIAP64, 2>(e.st.priv_ring, b * 2 * RO_E, 2 * RO_E, ring_s % 3, (int)threadIdx.x, RO_NT, hp);
        }
        if (pp.draws_out) {
            const int tile = 2 * b + (side ? 1 : 0);
            float* base = pp.draws_out + (int64_t)tile * pp.draws_len - lds_map(RO_E).u_delay;
            env_fill_draws<RO_E>(e, tile, (int)threadIdx.x, RO_NT, base, pp.in[0] + 1);
        }
        if (side) {
            phase_stamp(f.dbg, 1);
            if (e.out.obs_ahead) {
                hist_store<15, HGYM_OBS_FRAME, RO_NIA64, 2>(e.out.obs_ahead, b * 2 * RO_E, 2 * RO_E, ring_s % 15, (int)threadIdx.x, RO_NT, nullptr,
                                                            e.cfg.clip_obs, ha);
                hist_store<3, HGYM_PRIV_FRAME, RO_NIAP64, 2>(e.out.priv_ahead, b * 2 * RO_E, 2 * RO_E, ring_s % 3, (int)threadIdx.x, RO_NT, nullptr,
                                                             e.cfg.clip_obs, hp);
            }
            phase_stamp(f.dbg, 2);
            if (pp.ah.acc_out) l0_partial_ahead<2 * U, 2 * RO_E>(f.net[0], pp.ah, f.M, smem, b);
        }
        phase_stamp(f.dbg, 7);
        return;
    }
    if (critic_wg) {                                // critic tile
        // one instantiation only (first hidden layer 768 wide, rollout_fwd_args checks): with the three-way dispatch of
        // mlp_fwd_kernel next to the actor + env branch the compiler keeps a private-memory copy of the whole 3 KB argument
        fwd_body<32, 8, 4, 3 * U, false, false, false, GA>(f, f.net[1], false, smem);
        // rows after next of this tile (HGYM_RO_AHEAD_CRITIC): loads issued here, behind the tile, where the launch's first rush on memory is
        // over; they travel while the draws are computed; the stores' acknowledgements are waited for under the first-layer weights below
        float ha[RO_NIA_C][4], hp[RO_NIAP_C][4];
        const int ring_s = (int)pp.in[1];
        // (unconditional: the ring always exists; a launch without rows after next drops them)
        hist_load<15, HGYM_OBS_FRAME, RO_NIA_C, 2>(e.st.obs_ring, (int)blockIdx.x * RO_E, RO_E, ring_s % 15, (int)threadIdx.x, RO_NT, ha);
        hist_load<3, HGYM_PRIV_FRAME, RO_NIAP_C, 2>(e.st.priv_ring, (int)blockIdx.x * RO_E, RO_E, ring_s % 3, (int)threadIdx.x, RO_NT, hp);
        if (pp.draws_out) {      // next step's draw tables of this tile (step counter + 1), written where the LDS tables would be
            float* base = pp.draws_out + (int64_t)blockIdx.x * pp.draws_len - lds_map(RO_E).u_delay;
            env_fill_draws<RO_E>(e, (int)blockIdx.x, (int)threadIdx.x, RO_NT, base, pp.in[0] + 1);
        }
        if (e.out.obs_ahead) {
            hist_store<15, HGYM_OBS_FRAME, RO_NIA_C, 2>(e.out.obs_ahead, (int)blockIdx.x * RO_E, RO_E, ring_s % 15, (int)threadIdx.x, RO_NT, nullptr,
                                                        e.cfg.clip_obs, ha);
            hist_store<3, HGYM_PRIV_FRAME, RO_NIAP_C, 2>(e.out.priv_ahead, (int)blockIdx.x * RO_E, RO_E, ring_s % 3, (int)threadIdx.x, RO_NT, nullptr,
                                                         e.cfg.clip_obs, hp);
        }
        if (pp.ah.acc_out) {     // k-steps [0, kb0) of the ACTOR's first layer for the next step's rows of this tile
            __syncthreads();     // (the head wavefronts of this tile may still read its LDS)
            l0_partial_ahead<2 * U>(f.net[0], pp.ah, f.M, smem, (int)blockIdx.x);
        }
        phase_stamp(f.dbg, 7);
        return;
    }
    const int t = threadIdx.x, block = blockIdx.x;
    const int64_t csc0 = pp.in[0], ring_step = pp.in[1], sstep = pp.in[2];
    float* esm = reinterpret_cast<float*>(smem + pp.env_lds_off);
    float hist_o[RO_NIO][4], hist_p[RO_NIP][4];
    const int act_off = lds_map(RO_E).actions_in;
    const float* const draws_in = pp.draws_in ? pp.draws_in + (int64_t)block * pp.draws_len : nullptr;
    const int draws_len = pp.draws_len;
    auto early = [&](const EnvArgs& E) {
        env_reset_pose<RO_E>(E, t, RO_NT, esm);                       // one lane, under the tile's first loads
        // this step's draw tables, computed during the previous launch: a plain copy that travels with the tile's first loads
        // (plain float quads and unconditional clamped loads: a packed-struct array behind a condition is kept in private memory)
        float dq[2][4];
        const int dq4 = draws_len >> 2, dq_off = lds_map(RO_E).u_delay;
        const float* const dsrc = draws_in ? draws_in : E.st.commands;      // any readable address when there is nothing to copy
        const int dmax = draws_in ? dq4 - 1 : 0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = t + u * RO_NT;
            stage_ld(dq[u], dsrc + 4 * (i < dmax ? i : dmax));
        }
        if (t < 256) env_stage_in<RO_E, true>(E, block, t, 256, esm);      // travels with the tile's own first loads
        if (draws_in) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int i = t + u * RO_NT;
                if (i < dq4) stage_st(esm + dq_off + 4 * i, dq[u]);
            }
        }
    };
    auto mid = [&](const EnvArgs& E) {
        if (!PRE) hist_load<15, HGYM_OBS_FRAME, RO_NIO>(E.st.obs_ring, block * RO_E, RO_E, (int)(ring_step % 15), t, RO_NT, hist_o);
    };
    auto put = [&](int row, int j, float v) { esm[act_off + row * 12 + j] = v; };
    // the env step's Philox draws: on the six wavefronts that have no head block, while the other two compute the head
    auto idle = [&](const EnvArgs& E) {
        if (!draws_in) env_fill_draws<RO_E>(E, block, t - 128, RO_NT - 128, esm, csc0);
        // these lanes' share of the 14 older frames (in registers since `mid`) -> the stacked rows of the next observation, while
        // the two head wavefronts finish the tile: three quarters of that store phase leave the chain behind the tile
        if (!PRE) hist_store<15, HGYM_OBS_FRAME, RO_NIO>(E.out.obs, block * RO_E, RO_E, (int)(ring_step % 15), t, RO_NT, nullptr, E.cfg.clip_obs, hist_o);
    };
    if constexpr (EVAL) {
        // every lane of the two head wavefronts, with its row and its four head outputs (columns 4 q .. 4 q + 3 of the 16-column block)
        auto put_mu = [&](int wave, int, int, const float (&mu)[4]) {
            const int row = wave * 16 + (t & 15), q = (t & 63) >> 4;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (4 * q + c < HGYM_NUM_ACTIONS) esm[act_off + row * 12 + 4 * q + c] = mu[c];
        };
        fwd_body<32, 8, 4, 2 * U, false, false, false, GA>(f, f.net[0], false, smem, early, mid, FwdNoop(), e, idle, put_mu);      // (not `is_actor`: no sampling epilogue)
    } else {
        fwd_body<32, 8, 4, 2 * U, false, false, PART, GA>(f, f.net[0], true, smem, early, mid, put, e, idle, FwdNoop(), nullptr, nullptr, FwdNoop(), &pp.l0);
    }
    if (PART && f.net[0].xs) {
        // rows of this tile whose env was reset by the previous step: columns [0, 32 kb0) of their bf16 shadow were written ahead from
        // the un-reset history -- the row's older frames are zero now (the launch that reset them zeroed the fp32 row)
        const int pieces = 4 * pp.l0.kb0;           // 16-byte pieces per row
        for (int j = t; j < RO_E * pieces; j += RO_NT) {
            const int row = j / pieces, pc = j - row * pieces;
            const int m = block * RO_E + row;
            if (m < f.M && pp.l0.reset[m]) *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(f.net[0].xs + (int64_t)m * f.net[0].ldxs) + pc * 16) = (u32x4){0u, 0u, 0u, 0u};
        }
    }
    __syncthreads();                                // the tile's actions are in the env image; the policy buffers are dead
    // phase clock of the env part (hgym_prof_phase_buffer): the slots of grid row 2, which stamps nothing itself
    long long* dbg = f.dbg ? f.dbg + (int64_t)2 * gridDim.x * 8 + (int64_t)block * 8 : nullptr;
    auto stamp = [&](int slot) {
        if (dbg && t == 0) dbg[slot] = (long long)__builtin_amdgcn_s_memrealtime();
    };
    stamp(0);
    // did the previous step reset this lane's env of the tile?  Loaded HERE, consumed behind phase B: read there it
    // is a memory round trip at the very end of the workgroup
    const bool prev_rs = PRE && pp.prev_reset && (t & 63) < RO_E && pp.prev_reset[block * RO_E + (t & (RO_E - 1))] != 0;
    const EnvArgs& A = e;
    // the two older privileged frames (12 registers the policy tile could not spare): loaded here, stored behind the joints phase
    if (!PRE) hist_load<3, HGYM_PRIV_FRAME, RO_NIP>(A.st.priv_ring, block * RO_E, RO_E, (int)(ring_step % 3), t, RO_NT, hist_p);
    if (!PRE) {
        if (t < 128)          // the head wavefronts' share; the others stored theirs under the head (idle hook)
            hist_store<15, HGYM_OBS_FRAME, RO_NIO>(A.out.obs, block * RO_E, RO_E, (int)(ring_step % 15), t, RO_NT, nullptr, A.cfg.clip_obs, hist_o);
    }
    stamp(1);
    env_step_phase_j<RO_E, true>(A, block, t, RO_NT, esm);       // joints + per-joint reward products; synthetic-physics remainder on waves 6, 7
    if (!PRE)
        hist_store<3, HGYM_PRIV_FRAME, RO_NIP>(A.out.priv_obs, block * RO_E, RO_E, (int)(ring_step % 3), t, RO_NT, nullptr, A.cfg.clip_obs,
                                               hist_p);
    __syncthreads();
    stamp(2);
    if (t < RO_CHAIN) env_step_phase_a3<RO_E>(A, block, t, RO_NT, esm, csc0);      // the per-env chain, four wavefronts by role
    __syncthreads();
    env_step_phase_f<RO_E>(A, block, t, RO_NT, esm);       // per-joint reset / reference pose / frame entries / last_* copies
    env_step_reward_sum<RO_E>(A, block, t, RO_NT, esm);   // (the last wavefront: phase F has the first six)
    __syncthreads();
    stamp(3);
    env_stage_out<RO_E, true>(A, block, t, RO_NT, esm);
    stamp(4);
    env_step_phase_b<15, 3, RO_E>(A, block, t, RO_NT, esm, csc0, ring_step, false, true);
    if (PRE && pp.prev_reset) {
        // this launch's next-observation rows were pre-written by the previous launch from the history as IT found it: an env the previous
        // step reset has zero older frames (13 of 15, 1 of 3) -- every wavefront reads the tile's 32 flags, loops over the set ones
        const unsigned long long mask = __ballot(prev_rs);
        for (unsigned long long mm = mask; mm; mm &= mm - 1) {
            const int le = __builtin_ctzll(mm);
            float* dobs = A.out.obs + (int64_t)(block * RO_E + le) * 15 * HGYM_OBS_FRAME;
            float* dpriv = A.out.priv_obs + (int64_t)(block * RO_E + le) * 3 * HGYM_PRIV_FRAME;
            for (int i = t; i < 13 * HGYM_OBS_FRAME; i += RO_NT) dobs[i] = 0.0f;
            for (int i = t; i < HGYM_PRIV_FRAME; i += RO_NT) dpriv[i] = 0.0f;
        }
    }
    stamp(5);
    if (block == 0 && t == 0) {
        pp.out[0] = csc0 + 1;
        pp.out[1] = ring_step + 1;
        pp.out[2] = sstep + 1;
        if (A.out.t_step) A.out.t_step[0] = sstep + 1;     // the caller's sampling-step counter stays current
    }
}

template <bool FIN, bool PRE, bool PART = false, bool NOCRITIC = false, bool C64 = false, bool EVAL = false>
__global__ __launch_bounds__(RO_NT) void rollout_step_kernel(const FwdArgs f, const EnvArgs e, const FinArgs fin, const RolloutPP pp) {
    rollout_step_body<FIN, PRE, PART, NOCRITIC, C64, EVAL, false>(f, e, fin, pp);
}
// Any resolved activation: the forms without critic tiles (hgym_rollout_act.hip says why only those).
template <bool FIN, bool EVAL = false>
__global__ __launch_bounds__(RO_NT) void rollout_step_act_kernel(const FwdArgs f, const EnvArgs e, const FinArgs fin, const RolloutPP pp) {
    rollout_step_body<FIN, false, false, true, false, EVAL, true>(f, e, fin, pp);
}

// the forms of the launch (hgym_rollout_step / hgym_rollout_eval_step pick one; hgym_rollout_act.hip maps it to its instantiation)
enum RolloutForm { RO_NOCRITIC_FIRST = 0, RO_NOCRITIC_NEXT, RO_EVAL };
// hgym_rollout_act.hip: reserve the dynamic LDS of, and launch, rollout_step_act_kernel in `form`
int32_t launch_rollout_step_act(int form, dim3 grid, size_t lds, hipStream_t s, const FwdArgs& f, const EnvArgs& e, const FinArgs& fin,
                                const RolloutPP& pp);

}  // namespace hgym
