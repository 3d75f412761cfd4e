"""python humanoid-gym_amd/humanoid/scripts/train.py --task=humanoid_ppo --headless  (reference scripts/train.py:36-43).

Several GPUs of one node: the same command line under torch.distributed.run, one process per GPU --
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \\
           humanoid-gym_amd/humanoid/scripts/train.py --task=humanoid_ppo --headless --num_envs 4096
-- every rank owns --num_envs envs on its own GPU (its own env stream: helpers.shard_seed) and the ranks exchange [gradient | KL] once
per minibatch (algo/ppo/dist_utils.py); rank 0 alone logs and writes checkpoints (the replicas are bit-identical).

HGYM_EXACT_RESUME=1 sets the train config's `runner.exact_resume` attribute (not a key of the config classes, whose lists are the
reference's): every checkpoint gets an envstate_<it>.pt sidecar, and --resume from such a checkpoint continues the saved run bit
for bit instead of warm-starting a new one (OnPolicyRunner.load; one rank).

HGYM_DIAG_INTERVAL=<n> sets `runner.diag_interval` the same way: every n iterations PPO.diagnostics() runs behind the update (clip fraction,
KL, probability ratios, explained variance over the whole batch) and is logged as Diag/<key>; 0 or unset: never.

HGYM_NOISE_STD=log sets `policy.noise_std_type` the same way: the action noise is trained as log sigma (ActorCritic(noise_std_type="log"):
sigma = exp(log_std) cannot leave the positive numbers, the checkpoint's first entry is `log_std`); "scalar" or unset: the reference's `std`.

HGYM_SYMMETRY=1 sets `algorithm.symmetry` the same way: the update also trains on the left-right mirrored copy of every transition
(PPO.symmetry with XBot-L's tables, humanoid/utils/symmetry.py): minibatches twice as large, as many Adam steps.

HGYM_MIRROR_LOSS=<coef> sets `algorithm.mirror_loss_coef`: coef * mse(mu(s), mirror of mu(mirrored s)) joins the PPO loss (rsl_rl's
mirror_loss_coeff; XBot-L's tables are implied).  HGYM_SYMMETRY=1 still decides the augmentation: without it the minibatches keep their
size and the update pays one more actor forward.

HGYM_OBS_NORM=1 sets `policy.empirical_normalization` the same way: every observation column is standardised by running statistics
folded into the first layers (ActorCritic(empirical_normalization=True)); checkpoints carry the statistics.

HGYM_ADV_NORM=minibatch|none|batch sets `algorithm.advantage_normalization` the same way: the advantages standardised per minibatch
(rsl_rl's normalize_advantage_per_mini_batch), not at all, or -- "batch", unset: the reference's way -- once over the whole batch
(PPO.advantage_normalization).

HGYM_RND=<weight> sets `algorithm.rnd_cfg = {"weight": <weight>}` the same way: Random Network Distillation with its defaults and that
constant weight -- an intrinsic exploration reward added to the stored rewards ahead of GAE (PPO.rnd); checkpoints
carry rnd_state_dict.  Unset: off.

HGYM_SMOOTH=<lamT>[,<lamS>] sets `algorithm.smoothness_cfg = {"temporal_coef": lamT, "spatial_coef": lamS}`: the smoothness regulariser on
the policy's mean (PPO.smoothness), the spatial term's noise the env's own noise_scale_vec * noise_level.  Unset: off.  With HGYM_MIRROR_LOSS=<coef> and no HGYM_SYMMETRY both regularisers train at once, in one
actor head; with HGYM_SYMMETRY=1 the pair is refused.

HGYM_VALUE_NORM=1 sets `algorithm.value_normalization` the same way: the value targets standardised by running statistics of the returns, the
critic in normalised units (PPO.value_normalization); checkpoints carry value_norm_state_dict.  Unset: off.

HGYM_GUIDE_TEACHER=<model_*.pt> with HGYM_GUIDE=<coef>[,<final_step>] sets `algorithm.guidance_cfg = {"teacher": <path>, "coef": <coef>}` the
same way, with a final step also `"coef_schedule": {"mode": "linear", "initial_step": 0, "final_step": <final_step>, "final_value": 0}`: a
frozen teacher's cloning term inside the PPO loss, coef / (B A) sum (mu - mu_teacher)^2, its coefficient formed on the device and, with a
final step, decaying linearly to 0 over that many learning iterations, after which the update is the plain one again (PPO.guidance, DESIGN.md
section 33); checkpoints carry guidance_state_dict, so --resume needs no teacher file.  Both unset: off; exactly one set: ValueError.

HGYM_CRITIC_WARMUP=<n> sets `algorithm.critic_warmup_updates` the same way: the first n updates of the run move the value function alone
(PPO.critic_warmup_updates), for a checkpoint whose critic was never trained; 0 or unset: off.

HGYM_NOISE_COLOR=<beta> sets `algorithm.exploration_noise_cfg = {"kind": "colored", "beta": <beta>}` the same way, HGYM_NOISE_AR1=<rho> sets
`{"kind": "ar1", "rho": <rho>}`: the action noise of a rollout is temporally correlated instead of white (PPO.exploration_noise, DESIGN.md
section 35); 0.5 is the exponent "Colored Noise in PPO" recommends.  Both unset: off; both set: ValueError.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from humanoid.envs import *  # noqa: F401,F403,E402
from humanoid.utils import get_args, task_registry  # noqa: E402
from humanoid.utils.helpers import init_distributed  # noqa: E402


def guidance_cfg_from_env(environ):
    """HGYM_GUIDE_TEACHER / HGYM_GUIDE -> `algorithm.guidance_cfg`, or None when both are unset.  Exactly one set: guidance was asked for
    and cannot run -- ValueError, not a silently unguided run."""
    teacher, spec = environ.get("HGYM_GUIDE_TEACHER"), environ.get("HGYM_GUIDE")
    if bool(teacher) != bool(spec):
        raise ValueError("HGYM_GUIDE_TEACHER=%r and HGYM_GUIDE=%r: guidance needs both (a teacher checkpoint and <coef>[,<final_step>])" % (teacher, spec))
    if not teacher:
        return None
    g = spec.split(",")
    gc = {"teacher": teacher, "coef": float(g[0])}
    if len(g) > 1:
        gc["coef_schedule"] = {"mode": "linear", "initial_step": 0, "final_step": int(g[1]), "final_value": 0.0}
    return gc


def train(args):
    guidance_cfg_from_env(os.environ)      # (a half-set pair is refused before anything is built)
    from humanoid.algo.ppo.exploration_noise import config_from_env as noise_cfg_from_env
    noise_cfg = noise_cfg_from_env(os.environ)      # (both filters at once likewise)
    rank, world = init_distributed(args)
    env, env_cfg = task_registry.make_env(name=args.task, args=args)
    if os.environ.get("HGYM_EXACT_RESUME", "0") == "1":
        task_registry.get_cfgs(args.task)[1].runner.exact_resume = True
    if int(os.environ.get("HGYM_DIAG_INTERVAL", "0") or 0) > 0:
        task_registry.get_cfgs(args.task)[1].runner.diag_interval = int(os.environ["HGYM_DIAG_INTERVAL"])
    if os.environ.get("HGYM_NOISE_STD"):
        task_registry.get_cfgs(args.task)[1].policy.noise_std_type = os.environ["HGYM_NOISE_STD"]
    if os.environ.get("HGYM_SYMMETRY", "0") == "1":
        task_registry.get_cfgs(args.task)[1].algorithm.symmetry = True
    if float(os.environ.get("HGYM_MIRROR_LOSS", "0") or 0.0) != 0.0:
        task_registry.get_cfgs(args.task)[1].algorithm.mirror_loss_coef = float(os.environ["HGYM_MIRROR_LOSS"])
    if os.environ.get("HGYM_OBS_NORM", "0") == "1":
        task_registry.get_cfgs(args.task)[1].policy.empirical_normalization = True
    if os.environ.get("HGYM_ADV_NORM"):
        task_registry.get_cfgs(args.task)[1].algorithm.advantage_normalization = os.environ["HGYM_ADV_NORM"]
    if os.environ.get("HGYM_RND"):
        task_registry.get_cfgs(args.task)[1].algorithm.rnd_cfg = {"weight": float(os.environ["HGYM_RND"])}
    if os.environ.get("HGYM_SMOOTH"):
        lam = [float(x) for x in os.environ["HGYM_SMOOTH"].split(",")]
        task_registry.get_cfgs(args.task)[1].algorithm.smoothness_cfg = {"temporal_coef": lam[0], "spatial_coef": lam[1] if len(lam) > 1 else 0.0}
    if os.environ.get("HGYM_VALUE_NORM", "0") == "1":
        task_registry.get_cfgs(args.task)[1].algorithm.value_normalization = True
    if int(os.environ.get("HGYM_CRITIC_WARMUP", "0") or 0) > 0:      # PPO.critic_warmup_updates: the first n updates move the critic alone
        task_registry.get_cfgs(args.task)[1].algorithm.critic_warmup_updates = int(os.environ["HGYM_CRITIC_WARMUP"])
    if noise_cfg is not None:
        task_registry.get_cfgs(args.task)[1].algorithm.exploration_noise_cfg = noise_cfg
    gc = guidance_cfg_from_env(os.environ)
    if gc is not None:
        task_registry.get_cfgs(args.task)[1].algorithm.guidance_cfg = gc
    ppo_runner, train_cfg = task_registry.make_alg_runner(env=env, name=args.task, args=args, **({} if rank == 0 else {"log_root": None}))
    ppo_runner.learn(num_learning_iterations=train_cfg.runner.max_iterations, init_at_random_ep_len=True)
    if os.environ.get("HGYM_TRAIN_SIGNATURE"):      # tests: a signature of this rank's final parameters (replicas must agree bit for bit)
        import json
        import torch
        from hgym import _lib as L
        net = ppo_runner.alg.net
        bits = net.params.view(torch.int32).to(torch.int64)
        json.dump(dict(world=world, steps=int(float(net.opt_state[L.OPT_STEP])), lr=float(net.opt_state[L.OPT_LR]),
                       params=[int(bits.sum()), int((bits * (torch.arange(bits.numel(), device=bits.device) % 8191 + 1)).sum())],
                       comm=getattr(ppo_runner.alg, "comm_report", None)),
                  open(os.path.join(os.environ["HGYM_TRAIN_SIGNATURE"], "rank%d.json" % rank), "w"))
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.synchronize()
        if getattr(ppo_runner.alg, "_comm", None) is not None:
            ppo_runner.alg._comm.close()
        dist.barrier()
        dist.destroy_process_group()
    return ppo_runner


if __name__ == "__main__":
    train(get_args())
