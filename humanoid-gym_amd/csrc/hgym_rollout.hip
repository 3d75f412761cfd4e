// hgym_rollout.hip -- ONE launch per vec-step of the rollout: PPO.act, the env step and the previous step's finaliser.
//
// The rollout is a latency chain: [policy step -> env step] x 60, each link a kernel whose first act is
// a round trip to memory for its inputs and whose launch costs ~4 us before any wave runs.  Nothing in step t of env e depends
// on another env's step t -- the only cross-env pieces are the step finaliser's means, which already ride one launch behind
// (HgymEnvOut.defer_finalize).  So the two links are fused per env slice:
//
//   grid (N / 32, 2 [+ 1])    blockIdx.y = 0: ACTOR tile of 32 rows (mlp_fwd body, 8 wavefronts) and then the ENV STEP of the same
//                                            32 envs, fed with the tile's sampled actions through LDS;
//                             blockIdx.y = 1: CRITIC tile (values of the transition being collected);
//                             blockIdx.y = 2: the finaliser of the PREVIOUS env step, one workgroup.
//                             (rows 0 and 1 trade places on odd columns; in the steady-state launch the non-actor workgroups are
//                             64-row critic tiles and side-job workgroups instead, rollout_step_kernel below)
//
//   actor workgroup timeline  issue {bias, first weight k-steps, first input chunk} | issue the env step's state / sim loads |
//   Philox draws of the env step (ALU under all of those loads) | layer 0 | issue the loads of the 14 + 2 older history frames
//   of the 32 envs (registers; they have the rest of the tile to arrive) | layers 1, 2, head, sampling -> actions to HBM
//   (storage slot) and to LDS | older frames -> stacked outputs | joints | per-env chain (wavefront 0) | state write-back,
//   newest frame, reset fix-ups.
//
// The env phases are the functions of hgym_env_math.hpp that env_step_kernel runs (32 envs per workgroup, 512 lanes), so the
// arithmetic -- and hence every mask and every float -- is the unfused kernel's.  This translation unit is built with
// -ffp-contract=off like hgym_env.hip; hgym_fused.hpp restores the policy kernels' own setting for its part.
//
// Step counters.  env_step_kernel reads the common step counter / ring step from HgymEnvState::counters and the policy reads its
// sampling step from *step_counter; here the finaliser that bumps the former runs CONCURRENTLY (it belongs to the previous
// step), so the launch takes its three counters from a ping-pong record in the caller's scratch block: launch t reads
// pp[parity], workgroup (0, 0) writes pp[parity ^ 1] = pp[parity] + 1 for launch t + 1.  For the same reason the reset count
// and the episode-sum accumulators the finaliser consumes, and the rew / reset / time_out outputs it reads, are per parity:
// the caller hands two HgymEnvOut records (this step's, the previous step's) with distinct rew / reset / time_out buffers.
#define HGYM_TU_CONTRACT_OFF 1
#include "hgym_rollout.hpp"

namespace hgym {

__global__ void rollout_begin_kernel(const int64_t* __restrict__ counters, const int64_t* __restrict__ step, RolloutScratch* scr, int parity) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    scr->pp[parity][0] = counters[HGYM_CNT_STEP];
    scr->pp[parity][1] = counters[HGYM_CNT_RING];
    scr->pp[parity][2] = step[0];
}

__global__ __launch_bounds__(1024) void rollout_fin_kernel(const FinArgs f) { fin_block(f, threadIdx.x, blockDim.x); }

// Role layout of the launch's non-actor workgroups: 64-row critic tiles next to side-job workgroups (rollout_step_kernel) wherever the
// launch has critic tiles and the 32-row tiles pair up; HGYM_RO_CRITIC64=0 keeps the 32-row critic tiles that carry the side jobs
// themselves (A/B runs).  Both layouts compute the same bits.
static bool rollout_critic64(int M, bool nocritic) {
    const char* v = getenv("HGYM_RO_CRITIC64");       // (read per call, as HGYM_L0_KB0)
    if (v && atoi(v) == 0) return false;
    return !nocritic && M >= 4 * RO_E && (M / RO_E) % 2 == 0;
}

static FinArgs parity_fin(const HgymEnvConfig& cfg, const HgymEnvState& st, const HgymEnvOut& out, RolloutScratch* scr, int parity) {
    FinArgs f = make_fin_args(cfg, st, out, FIN_MODE_STEP);
    f.reset_count = &scr->reset_cnt[parity];
    f.episode_acc = scr->acc[parity];
    return f;
}

}  // namespace hgym

using namespace hgym;

extern "C" {

int32_t hgym_rollout_begin(const HgymEnvState* st, const int64_t* step_counter, void* scratch, int32_t parity, void* stream) {
    HG_REQUIRE(st && st->counters && step_counter && scratch, HGYM_E_BADARG, "null state / step counter / scratch");
    HG_REQUIRE(parity == 0 || parity == 1, HGYM_E_BADARG, "parity=%d", parity);
    hipLaunchKernelGGL(rollout_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, st->counters, step_counter, (RolloutScratch*)scratch,
                       parity);
    HG_CHECK_LAUNCH("rollout_begin_kernel");
    return HGYM_OK;
}

int32_t hgym_rollout_step(const HgymNetConfig* cfg, const HgymNet* net, const HgymEnvConfig* env_cfg, const HgymSimTensors* sim,
                          const HgymEnvState* st, const HgymEnvOut* out, const HgymEnvOut* prev_out, const float* obs, const float* priv,
                          uint64_t seed, float* actions, float* mu, float* sigma, float* logp, float* values, void* scratch,
                          int32_t parity, const HgymObsShadow* shadow, void* stream) {
    return hgym_rollout_step_z(cfg, net, env_cfg, sim, st, out, prev_out, obs, priv, seed, actions, mu, sigma, logp, values, scratch, parity,
                               shadow, stream, nullptr);
}

// hgym_rollout_step with this step's (num_envs, 12) normals in place of the actor epilogue's own draw (a row of hgym_policy_noise_table's
// table): the same kernels, launched with FwdArgs.z set -- a host-side difference only.  z = NULL: hgym_rollout_step itself.
int32_t hgym_rollout_step_z(const HgymNetConfig* cfg, const HgymNet* net, const HgymEnvConfig* env_cfg, const HgymSimTensors* sim,
                            const HgymEnvState* st, const HgymEnvOut* out, const HgymEnvOut* prev_out, const float* obs, const float* priv,
                            uint64_t seed, float* actions, float* mu, float* sigma, float* logp, float* values, void* scratch,
                            int32_t parity, const HgymObsShadow* shadow, void* stream, const float* z) {
    HG_REQUIRE(cfg && net && env_cfg && sim && st && out && scratch, HGYM_E_BADARG, "null argument");
    HG_REQUIRE(((uintptr_t)z & 3) == 0, HGYM_E_BADARG, "z must be 4-byte aligned");
    const bool nocritic = values == nullptr;      // deferred values (header v7): hgym_critic_values runs after the rollout
    HG_REQUIRE(obs && actions && mu && sigma && logp && (nocritic || priv), HGYM_E_BADARG, "null policy buffer");
    HG_REQUIRE(parity == 0 || parity == 1, HGYM_E_BADARG, "parity=%d", parity);
    // what the kernel compiles in (the header's "Supported:" list): the actor epilogue writes 12 actions per row into the env image
    // and the env part produces 15 x 47 / 3 x 73 wide rows, which the policy tiles read with these leading dimensions
    HG_REQUIRE(cfg->num_actions == HGYM_NUM_ACTIONS && cfg->num_obs == 15 * HGYM_OBS_FRAME && cfg->num_priv == 3 * HGYM_PRIV_FRAME,
               HGYM_E_UNSUPPORTED, "fused rollout step: net shape %d / %d -> %d is not XBot-L's 705 / 219 -> 12", cfg->num_obs, cfg->num_priv,
               cfg->num_actions);
    RolloutScratch* scr = (RolloutScratch*)scratch;
    const int M = env_cfg->num_envs;
    FwdArgs f;
    EnvArgs e;
    FinArgs fin;
    RolloutPP pp;
    memset(&fin, 0, sizeof(fin));
    pp.prev_reset = nullptr;
    size_t lds_pol = 0;
    int32_t rc = rollout_fwd_args(cfg, net, M, obs, priv, seed, &scr->pp[parity][2], actions, mu, sigma, logp, values, &f, &lds_pol, shadow, z);
    if (rc) return rc;
    rc = rollout_env_args(env_cfg, sim, st, out, actions, &e);
    if (rc) return rc;
    HG_REQUIRE(out->t_values == values, HGYM_E_BADARG, "the transition sink must take this launch's values");
    if (nocritic) {
        HG_REQUIRE(out->t_rewards && out->t_time_outs && (!prev_out || (prev_out->t_time_outs && !prev_out->t_values)), HGYM_E_BADARG,
                   "values = NULL: the transition sinks must be of the deferred kind (t_values NULL, t_time_outs set)");
        HG_REQUIRE(!out->obs_ahead && !out->priv_ahead && !out->obs_older_ready && !out->l0_ahead && !out->l0_ready && !out->obs_bf16_ahead,
                   HGYM_E_BADARG, "values = NULL: rows ahead / the carried first layer are the critic workgroups' side jobs");
    }
    e.reset_count = &scr->reset_cnt[parity];
    e.st.episode_acc = scr->acc[parity];
    if (prev_out) {
        HG_REQUIRE(prev_out->rew != out->rew && prev_out->reset != out->reset && prev_out->time_out != out->time_out, HGYM_E_BADARG,
                   "this step's and the previous step's rew / reset / time_out must be distinct buffers (the finaliser runs concurrently)");
        HG_REQUIRE(prev_out->time_out && prev_out->extras_time_outs && prev_out->extras_episode && prev_out->rew && prev_out->reset,
                   HGYM_E_BADARG, "null finaliser buffer");
        fin = parity_fin(*env_cfg, *st, *prev_out, scr, parity ^ 1);
        pp.prev_reset = prev_out->reset;
    }
    pp.in = scr->pp[parity];
    pp.out = scr->pp[parity ^ 1];
    pp.env_lds_off = (int)round_up((int64_t)lds_pol, 16);
    {   // draw tables handed from launch to launch: [parity][tile][draws_len] floats behind the scratch header
        const LdsMap m = lds_map(RO_E);
        pp.draws_len = m.frame - m.u_delay;
        HG_REQUIRE((pp.draws_len & 3) == 0 && (m.u_delay & 3) == 0 && pp.draws_len <= 2 * 4 * RO_NT &&
                       (size_t)pp.draws_len * 4 * 2 <= (size_t)HGYM_ROLLOUT_DRAW_BYTES_PER_ENV * RO_E,
                   HGYM_E_UNSUPPORTED, "draw tables of %d floats per tile do not fit the scratch layout", pp.draws_len);
        float* tables = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + HGYM_ROLLOUT_SCRATCH_HEADER_BYTES);
        const int64_t per_parity = (int64_t)(M / RO_E) * pp.draws_len;
        pp.draws_in = (prev_out && !nocritic) ? tables + parity * per_parity : nullptr;       // the first step of a rollout draws its own
        pp.draws_out = nocritic ? nullptr : tables + (parity ^ 1) * per_parity;
    }
    memset(&pp.l0, 0, sizeof(pp.l0));
    memset(&pp.ah, 0, sizeof(pp.ah));
    const bool part = out->l0_ready != nullptr;
    // the layout is chosen per env count, so that the k-steps carried ahead agree between the launch that forms them and the next;
    // the steady-state launch (part) runs it, the first launch of a rollout keeps the 32-row critic tiles
    const bool elu1 = act_is_elu1(f.act);      // else: rollout_step_act_kernel, which exists without critic tiles only (hgym_rollout_act.hip)
    HG_REQUIRE(elu1 || nocritic, HGYM_E_UNSUPPORTED, "fused rollout step with an activation other than ELU(1): the deferred form only (values = NULL, "
               "the critic once after the rollout: hgym_critic_values) -- the forms with critic tiles would exceed the per-kernel code limit");
    const bool critic64 = elu1 && rollout_critic64(M, nocritic);
    const bool c64 = critic64 && part;
    int kb0_ahead = 0;
    {   // first layer of the actor carried across launches (HgymEnvOut.l0_ahead / l0_ready)
        // k-steps formed ahead: whole 128-column chunks, at most 20 (640 of the 658 columns of the 14 older frames).  With 32-row critic
        // tiles 12 by default: the critic workgroup pays for every k-step it takes over at the same L2 -> CU fill rate, and with all 20
        // it becomes the launch's longest workgroup (profiles/r04_l0_ahead_ab.txt: collection 2.33 -> 2.27 ms with 12, 2.30 with 20,
        // 2.34 with 8).  With 64-row critic tiles the side-job workgroup carries them, one weight stream for two actor tiles: all 20
        // (DESIGN.md section 13).  HGYM_L0_KB0 tunes the split (A/B runs).
        const int kb0_def = critic64 ? 20 : 12;
        const char* kb0_env = getenv("HGYM_L0_KB0");          // (read per call: the tests run several splits in one process)
        const int kb0_v = kb0_env ? atoi(kb0_env) : kb0_def;
        const int KB0_AHEAD = (kb0_v >= 4 && kb0_v <= 20 && kb0_v % 4 == 0) ? kb0_v : kb0_def;
        kb0_ahead = KB0_AHEAD;
        HG_REQUIRE(!part || prev_out, HGYM_E_BADARG, "l0_ready on the first step of a rollout: no launch has left partial sums");
        HG_REQUIRE(!(part || out->l0_ahead) || (f.net[0].layer[0].KB == 24 && f.net[0].layer[0].N == 512 && HGYM_OBS_FRAME * 14 >= 32 * KB0_AHEAD),
                   HGYM_E_UNSUPPORTED, "the carried first layer is built for XBot-L's 15 x 47 -> 512 actor input");
        // the consuming tile runs k-steps [kb0, KR): at least one of them (its last-chunk form takes 1..4)
        HG_REQUIRE(!(part || out->l0_ahead) || KB0_AHEAD <= f.net[0].layer[0].KR - 1, HGYM_E_UNSUPPORTED,
                   "the carried first layer: %d k-steps ahead of the %d the input width needs", KB0_AHEAD, f.net[0].layer[0].KR);
        HG_REQUIRE(!out->l0_ahead || (((uintptr_t)out->l0_ahead & 15) == 0 && out->l0_ahead != out->l0_ready), HGYM_E_BADARG,
                   "l0_ahead must be 16-byte aligned and distinct from l0_ready");
        HG_REQUIRE(!out->obs_bf16_ahead || (out->l0_ahead && out->ld_obs_bf16_ahead >= 768 && out->ld_obs_bf16_ahead % 8 == 0 &&
                                           ((uintptr_t)out->obs_bf16_ahead & 15) == 0), HGYM_E_BADARG, "obs_bf16_ahead: needs l0_ahead, ld >= 768 (multiple of 8), 16-byte aligned");
        if (part) {
            pp.l0.acc = out->l0_ready;
            pp.l0.reset = prev_out->reset;
            pp.l0.kb0 = KB0_AHEAD;
        }
        if (out->l0_ahead) {
            pp.ah.acc_out = out->l0_ahead;
            pp.ah.xs_next = (__bf16*)out->obs_bf16_ahead;
            pp.ah.ldxs = out->ld_obs_bf16_ahead;
            pp.ah.shift = HGYM_OBS_FRAME;
            pp.ah.kb0 = KB0_AHEAD;
        }
    }
    f.dbg = phase_buffer((int64_t)(M / RO_E) * 3);
    size_t lds = (size_t)pp.env_lds_off + step_smem_bytes(RO_E);
    if (c64) {               // the 64-row critic tile's buffers; the side jobs' first-layer staging (64 rows x 32 kb0 bf16 columns)
        lds = std::max(lds, (size_t)fwd_lds_bytes(f.net[1], 2 * RO_E));
        if (out->l0_ahead) lds = std::max(lds, (size_t)2 * RO_E * 32 * kb0_ahead * 2);
    }
    const bool pre = out->obs_older_ready != 0;
    HG_REQUIRE(!pre || prev_out, HGYM_E_BADARG, "obs_older_ready on the first step of a rollout: no launch has written those frames");
    HG_REQUIRE(!part || pre, HGYM_E_UNSUPPORTED, "l0_ready is built together with obs_older_ready (the steady-state launch)");
    HG_REQUIRE((out->obs_ahead != nullptr) == (out->priv_ahead != nullptr), HGYM_E_BADARG, "obs_ahead and priv_ahead: both or neither");
    HG_REQUIRE(!out->obs_ahead || (out->obs_ahead != out->obs && out->priv_ahead != out->priv_obs), HGYM_E_BADARG,
               "obs_ahead / priv_ahead must be the rows AFTER obs / priv_obs");
    if (elu1) {
        const void* fn = nocritic ? (prev_out ? reinterpret_cast<const void*>(&rollout_step_kernel<true, false, false, true>)
                                              : reinterpret_cast<const void*>(&rollout_step_kernel<false, false, false, true>))
                       : c64 ? reinterpret_cast<const void*>(&rollout_step_kernel<true, true, true, false, true>)
                       : part ? reinterpret_cast<const void*>(&rollout_step_kernel<true, true, true>)
                       : pre ? reinterpret_cast<const void*>(&rollout_step_kernel<true, true>)
                             : (prev_out ? reinterpret_cast<const void*>(&rollout_step_kernel<true, false>)
                                         : reinterpret_cast<const void*>(&rollout_step_kernel<false, false>));
        rc = ensure_dynamic_lds(fn, lds, "rollout_step_kernel");
        if (rc) return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    prof_begin(HGYM_PROF_ROLLOUT, s);
    if (!elu1) {
        rc = launch_rollout_step_act(prev_out ? RO_NOCRITIC_NEXT : RO_NOCRITIC_FIRST, dim3(M / RO_E, prev_out ? 2 : 1), lds, s, f, e, fin, pp);
        if (rc) return rc;
    } else if (nocritic && prev_out) hipLaunchKernelGGL((rollout_step_kernel<true, false, false, true>), dim3(M / RO_E, 2), dim3(RO_NT), lds, s, f, e, fin, pp);
    else if (nocritic) hipLaunchKernelGGL((rollout_step_kernel<false, false, false, true>), dim3(M / RO_E, 1), dim3(RO_NT), lds, s, f, e, fin, pp);
    else if (c64) hipLaunchKernelGGL((rollout_step_kernel<true, true, true, false, true>), dim3(M / RO_E, 3), dim3(RO_NT), lds, s, f, e, fin, pp);
    else if (part) hipLaunchKernelGGL((rollout_step_kernel<true, true, true>), dim3(M / RO_E, 3), dim3(RO_NT), lds, s, f, e, fin, pp);
    else if (pre) hipLaunchKernelGGL((rollout_step_kernel<true, true>), dim3(M / RO_E, 3), dim3(RO_NT), lds, s, f, e, fin, pp);
    else if (prev_out) hipLaunchKernelGGL((rollout_step_kernel<true, false>), dim3(M / RO_E, 3), dim3(RO_NT), lds, s, f, e, fin, pp);
    else hipLaunchKernelGGL((rollout_step_kernel<false, false>), dim3(M / RO_E, 2), dim3(RO_NT), lds, s, f, e, fin, pp);
    {   // algorithmic HBM bytes of the fused step: the env step's + the policy's input rows and outputs
        // + the policy's weights, read once per launch (3 704 420 B / N per env-step in fp32 terms; here the bf16 forward
        // fragments the tiles actually stream, padded layout) -- until round 4 this term was left out (0.149 -> 0.155 at N = 4096)
        const double env_b = 4.0 * (245 + 14 * 47 + 2 * 73 + 15 * 47 + 3 * 73) + 6;
        const double pol_b = 4.0 * (cfg->num_obs + cfg->num_priv + 3 * cfg->num_actions + 2);
        double w_b = 0.0;
        for (int n = 0; n < (nocritic ? 1 : 2); ++n)
            for (int l = 0; l < 4; ++l) w_b += (double)f.net[n].layer[l].NB * f.net[n].layer[l].KB * 1024.0;
        // (deferred values: the critic's input rows, its value and its weights are hgym_critic_values' bytes, not this launch's)
        prof_end(HGYM_PROF_ROLLOUT, s, (double)M * (env_b + pol_b - (nocritic ? 4.0 * (cfg->num_priv + 1) : 0.0)) + w_b);
    }
    HG_CHECK_LAUNCH("rollout_step_kernel");
    return HGYM_OK;
}

int32_t hgym_rollout_eval_step(const HgymNetConfig* cfg, const HgymNet* net, const HgymEnvConfig* env_cfg, const HgymSimTensors* sim,
                               const HgymEnvState* st, const HgymEnvOut* out, const HgymEnvOut* prev_out, const float* obs, float* actions,
                               void* scratch, int32_t parity, void* stream) {
    HG_REQUIRE(cfg && net && env_cfg && sim && st && out && scratch && obs && actions, HGYM_E_BADARG, "null argument");
    HG_REQUIRE(parity == 0 || parity == 1, HGYM_E_BADARG, "parity=%d", parity);
    HG_REQUIRE(cfg->num_actions == HGYM_NUM_ACTIONS && cfg->num_obs == 15 * HGYM_OBS_FRAME, HGYM_E_UNSUPPORTED,
               "fused evaluation step: actor shape %d -> %d is not XBot-L's 705 -> 12", cfg->num_obs, cfg->num_actions);
    HG_REQUIRE(!out->t_rewards && !out->t_values && !out->t_dones && !out->t_step && !out->t_time_outs && !out->log_stats && out->defer_finalize,
               HGYM_E_BADARG, "the evaluation step stores no transition and keeps no training log: sinks NULL, defer_finalize = 1");
    HG_REQUIRE(!out->obs_ahead && !out->priv_ahead && !out->obs_older_ready && !out->l0_ahead && !out->l0_ready && !out->obs_bf16_ahead,
               HGYM_E_BADARG, "rows ahead / the carried first layer do not exist in the evaluation launch");
    HG_REQUIRE(out->obs != obs, HGYM_E_BADARG, "the next observation rows must not be the rows this launch reads");
    RolloutScratch* scr = (RolloutScratch*)scratch;
    const int M = env_cfg->num_envs;
    FwdArgs f;
    EnvArgs e;
    FinArgs fin;
    RolloutPP pp;
    memset(&fin, 0, sizeof(fin));
    memset(&pp, 0, sizeof(pp));
    size_t lds_pol = 0;
    int32_t rc = rollout_eval_fwd_args(cfg, net, M, obs, actions, &f, &lds_pol);
    if (rc) return rc;
    rc = rollout_env_args(env_cfg, sim, st, out, actions, &e, false);
    if (rc) return rc;
    e.reset_count = &scr->reset_cnt[parity];
    e.st.episode_acc = scr->acc[parity];
    if (prev_out) {
        HG_REQUIRE(prev_out->rew != out->rew && prev_out->reset != out->reset && prev_out->time_out != out->time_out, HGYM_E_BADARG,
                   "this step's and the previous step's rew / reset / time_out must be distinct buffers (the finaliser runs concurrently)");
        HG_REQUIRE(prev_out->time_out && prev_out->extras_time_outs && prev_out->extras_episode && prev_out->rew && prev_out->reset &&
                       !prev_out->t_rewards && !prev_out->log_stats, HGYM_E_BADARG, "null finaliser buffer, or a sink in prev_out");
        fin = parity_fin(*env_cfg, *st, *prev_out, scr, parity ^ 1);
    }
    pp.in = scr->pp[parity];
    pp.out = scr->pp[parity ^ 1];
    pp.env_lds_off = (int)round_up((int64_t)lds_pol, 16);
    {
        const LdsMap m = lds_map(RO_E);
        pp.draws_len = m.frame - m.u_delay;       // (no tables are handed over: every workgroup draws its own step's numbers)
    }
    f.dbg = nullptr;
    const size_t lds = (size_t)pp.env_lds_off + step_smem_bytes(RO_E);
    // grid row 1 = the previous step's finaliser; the first launch of an evaluation has none and is launched without that row
    if (!act_is_elu1(f.act)) {
        rc = launch_rollout_step_act(RO_EVAL, dim3(M / RO_E, prev_out ? 2 : 1), lds, (hipStream_t)stream, f, e, fin, pp);
        if (rc) return rc;
        HG_CHECK_LAUNCH("rollout_step_act_kernel (evaluation)");
        return HGYM_OK;
    }
    rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&rollout_step_kernel<true, false, false, true, false, true>), lds, "rollout_step_kernel (evaluation)");
    if (rc) return rc;
    hipLaunchKernelGGL((rollout_step_kernel<true, false, false, true, false, true>), dim3(M / RO_E, prev_out ? 2 : 1), dim3(RO_NT), lds,
                       (hipStream_t)stream, f, e, fin, pp);
    HG_CHECK_LAUNCH("rollout_step_kernel (evaluation)");
    return HGYM_OK;
}

int32_t hgym_rollout_end(const HgymEnvConfig* env_cfg, const HgymEnvState* st, const HgymEnvOut* last_out, void* scratch, int32_t parity,
                         void* stream) {
    HG_REQUIRE(env_cfg && st && last_out && scratch, HGYM_E_BADARG, "null argument");
    HG_REQUIRE(parity == 0 || parity == 1, HGYM_E_BADARG, "parity=%d", parity);
    HG_REQUIRE(st->counters && last_out->time_out && last_out->extras_time_outs && last_out->extras_episode && last_out->rew && last_out->reset,
               HGYM_E_BADARG, "null finaliser buffer");
    const FinArgs f = parity_fin(*env_cfg, *st, *last_out, (RolloutScratch*)scratch, parity);
    hipLaunchKernelGGL(rollout_fin_kernel, dim3(1), dim3(env_cfg->num_envs > 256 ? 1024 : 256), 0, (hipStream_t)stream, f);
    HG_CHECK_LAUNCH("rollout_fin_kernel");
    return HGYM_OK;
}

}  // extern "C"
