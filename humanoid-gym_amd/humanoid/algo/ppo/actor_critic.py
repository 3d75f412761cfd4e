"""ActorCritic with the reference's interface and state_dict keys (algo/ppo/actor_critic.py:36-128):
`std`, `actor.{0,2,4,6}.{weight,bias}`, `critic.{0,2,4,6}.{weight,bias}`.

The module is an ordinary nn.Module so checkpoints, `copy.deepcopy(actor_critic.actor)` + TorchScript export
(utils/helpers.py export_policy_as_jit) and CPU inference of the exported actor keep working.  For training,
`bind()` re-points every parameter at its slice of the flat fp32 master vector of a hgym.NetBuffers, after which
act / evaluate / log-prob run through libhgym_hip.so (MFMA forward, fused Gaussian epilogue) and the optimiser
kernels update the very memory the module's parameters alias.
"""
import math
import os

import torch
import torch.nn as nn

_HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def _mlp(sizes, activation):
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            layers.append(activation)
    return nn.Sequential(*layers)


class ActorCritic(nn.Module):
    def __init__(self, num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=[256, 256, 256],
                 critic_hidden_dims=[256, 256, 256], init_noise_std=1.0, activation=nn.ELU(), denoiser_hidden_dims=None,
                 denoiser_targets=0, fused_activation=None, noise_std_type="scalar", empirical_normalization=False,
                 normalization_eps=1e-2, normalization_until=None, **kwargs):
        """denoiser_hidden_dims / denoiser_targets (native extension, BASELINE configs[4]): an auxiliary head
        obs -> denoiser_hidden_dims -> denoiser_targets that regresses the newest `denoiser_targets` columns of the
        privileged observation (the clean single-frame privileged state) from the noisy observation history; trained jointly
        with PPO (PPO(denoise_coef=...)).  The reference has no code for it (README.md:113); off by default.
        fused_activation (native extension): run the fused bf16 kernels with `activation` whatever it is, not only with ELU(1)
        (HgymNetConfig.fused_activation; PPO passes it into the net config).  None: the environment variable HGYM_FUSED_ACT ("1": on),
        else off.
        noise_std_type (as in current rsl_rl): "scalar" -- the reference's parameter `std`, the standard deviations themselves, which
        nothing keeps positive -- or "log" -- the parameter is `log_std` (first in the state dict, where `std` is otherwise) and
        sigma = exp(log_std) stays positive wherever the optimiser moves it.  `noise_std` is sigma in both modes.
        empirical_normalization (as in current rsl_rl): every observation column of the actor, the critic and the denoiser head is
        standardised by a running mean and standard deviation, (x - mean) / (std + normalization_eps) -- here as part of the first
        layer: the kernels read raw rows and the statistics are folded into the first-layer operands.  The
        statistics are updated once per PPO.update(), from the rollout it trained on (rsl_rl: at every env step), until
        `normalization_until` rows have been seen (None: always).  `obs_normalizer` / `critic_obs_normalizer` expose them
        (nn.Identity() when off).  The parameters, the state dict and the optimiser stay in the normalised parametrisation."""
        from hgym.net import activation_spec, std_param_spec, check_obs_norm
        std_param_spec(noise_std_type)       # ValueError for anything but "scalar" / "log", before anything is built
        normalization_eps, normalization_until = check_obs_norm(normalization_eps, normalization_until)      # ValueError: eps < 0, until < 0
        if kwargs:
            print("ActorCritic.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs.keys())))
        super().__init__()
        activation_spec(activation)          # NotImplementedError (listing what is supported) for anything the kernels lack
        self.activation = activation
        self.fused_activation = (os.environ.get("HGYM_FUSED_ACT", "0") == "1") if fused_activation is None else bool(fused_activation)
        self.num_actor_obs, self.num_critic_obs, self.num_actions = num_actor_obs, num_critic_obs, num_actions
        self.actor_hidden_dims, self.critic_hidden_dims = list(actor_hidden_dims), list(critic_hidden_dims)
        self.actor = _mlp([num_actor_obs] + self.actor_hidden_dims + [num_actions], activation)
        self.critic = _mlp([num_critic_obs] + self.critic_hidden_dims + [1], activation)
        self.denoiser_hidden_dims = list(denoiser_hidden_dims) if denoiser_hidden_dims else None
        self.denoiser_targets = int(denoiser_targets) if self.denoiser_hidden_dims else 0
        if self.denoiser_hidden_dims:
            self.denoiser = _mlp([num_actor_obs] + self.denoiser_hidden_dims + [self.denoiser_targets], activation)
        print(f"Actor MLP: {self.actor}")
        print(f"Critic MLP: {self.critic}")
        self.noise_std_type = noise_std_type
        if noise_std_type == "log":
            self.log_std = nn.Parameter(torch.log(init_noise_std * torch.ones(num_actions)))
        else:
            self.std = nn.Parameter(init_noise_std * torch.ones(num_actions))
        self.empirical_normalization = bool(empirical_normalization)
        self.normalization_eps, self.normalization_until = normalization_eps, normalization_until
        if self.empirical_normalization:
            from .normalizer import EmpiricalNormalization
            self.obs_normalizer = EmpiricalNormalization(num_actor_obs, normalization_eps, normalization_until, which=0)
            self.critic_obs_normalizer = EmpiricalNormalization(num_critic_obs, normalization_eps, normalization_until, which=1)
        else:
            self.obs_normalizer, self.critic_obs_normalizer = nn.Identity(), nn.Identity()
        self._net = None          # hgym.NetBuffers once bound
        self._last = None         # outputs of the last act(): mu, sigma, logp, values
        self._sample_seed = 0
        self._sample_step = None

    # ------------------------------------------------------------------ binding to the HIP path
    def bind(self, net):
        """Alias every parameter to its slice of net.params (state_dict order) and keep them in sync."""
        with torch.no_grad():
            for name, p in self.named_parameters():
                view = net.views[name]
                view.copy_(p.detach().to(view.device))
                p.data = view
        self._net = net
        if self.empirical_normalization:
            if getattr(net, "obs_norm", None) is None:
                raise RuntimeError("ActorCritic(empirical_normalization=True) bound to a NetBuffers built without obs_norm")
            self.obs_normalizer.bind(net)
            self.critic_obs_normalizer.bind(net)
        net.sync_shadow()
        return self

    @property
    def obs_norm_spec(self):
        """NetBuffers' obs_norm argument: (eps, until), or None when empirical_normalization is off."""
        return (self.normalization_eps, self.normalization_until) if self.empirical_normalization else None

    def norm_state_dicts(self):
        """{"obs_norm_state_dict": ..., "critic_obs_norm_state_dict": ...} for a checkpoint; {} when normalisation is off."""
        if not self.empirical_normalization:
            return {}
        return dict(obs_norm_state_dict=self.obs_normalizer.norm_state_dict(),
                    critic_obs_norm_state_dict=self.critic_obs_normalizer.norm_state_dict())

    def folded_first_layer(self, which=0):
        """(W o s, b') in fp32 on the cpu: the first layer of the actor (0), critic (1) or denoiser (2) that takes RAW observations --
        what an exported policy carries.  b' = b - (W o s) m in float64, rounded once.  Without normalisation: the layer itself."""
        seq = (self.actor, self.critic, getattr(self, "denoiser", None))[which]
        W, b = seq[0].weight.detach().cpu().float(), seq[0].bias.detach().cpu().float()
        if not self.empirical_normalization:
            return W.clone(), b.clone()
        nz = self.critic_obs_normalizer if which == 1 else self.obs_normalizer
        m = nz.mean.cpu().float()
        sc = (1.0 / (torch.sqrt(nz.var.cpu()) + float(torch.tensor(nz.eps, dtype=torch.float32)))).float()
        Ws = W * sc[None, :]
        return Ws, (b.double() - (Ws.double() * m.double()[None, :]).sum(dim=1)).float()

    @property
    def bound(self):
        return self._net is not None

    def load_state_dict(self, state_dict, strict=True):
        out = super().load_state_dict(state_dict, strict=strict)
        if self._net is not None:
            self._net.sync_shadow()
        return out

    def _need_net(self):
        if self._net is None:
            raise RuntimeError("ActorCritic is not bound to the HIP network (PPO binds it); there is no CPU training path")
        return self._net

    # ------------------------------------------------------------------ reference API
    @staticmethod
    def init_weights(sequential, scales):
        [torch.nn.init.orthogonal_(m.weight, gain=scales[i]) for i, m in
         enumerate(mod for mod in sequential if isinstance(mod, nn.Linear))]

    def reset(self, dones=None):
        pass

    def forward(self):
        raise NotImplementedError

    @property
    def noise_std(self):
        """The num_actions standard deviations, whichever way they are parametrised."""
        if self.noise_std_type != "log":
            return self.std.detach()
        return self._net.sigma if self._net is not None else torch.exp(self.log_std.detach())

    @property
    def action_mean(self):
        return self._last["mu"]

    @property
    def action_std(self):
        return self._last["sigma"]

    @property
    def entropy(self):
        return (0.5 + _HALF_LOG_2PI + torch.log(self._last["sigma"])).sum(dim=-1)

    def update_distribution(self, observations):
        net = self._need_net()
        mu = net.forward(0, observations.contiguous())
        self._last = dict(mu=mu, sigma=mu * 0.0 + self.noise_std)

    def act(self, observations, critic_observations=None, out=None, env_fin=None, shadow=None, z=None, **kwargs):
        """Sample actions.  With critic_observations the critic runs in the same call (what PPO.act needs).  z (native extension):
        (M, num_actions) standard normals in place of the launch's own draw (PPO.exploration_noise)."""
        net = self._need_net()
        if critic_observations is None:
            self.update_distribution(observations)
            z = torch.randn_like(self._last["mu"]) if z is None else z
            a = self._last["mu"] + self._last["sigma"] * z
            self._last["actions"] = a
            return a
        self._last = net.act(observations.contiguous(), critic_observations.contiguous(), seed=self._sample_seed,
                             step_counter=self._sample_step, out=out, env_fin=env_fin, shadow=shadow, z=z)
        return self._last["actions"]

    def get_actions_log_prob(self, actions):
        if self._last is not None and self._last.get("actions") is actions and "logp" in self._last:
            return self._last["logp"]
        mu, sg = self._last["mu"], self._last["sigma"]
        return (-((actions - mu) ** 2) / (2 * sg ** 2) - torch.log(sg) - _HALF_LOG_2PI).sum(dim=-1)

    def act_inference(self, observations):
        if self._net is not None and observations.is_cuda:
            return self._net.forward(0, observations.contiguous())
        return self.actor(self.obs_normalizer(observations))        # exported-policy / CPU evaluation plumbing (BASELINE config #1)

    def evaluate(self, critic_observations, **kwargs):
        return self._need_net().forward(1, critic_observations.contiguous())

    def denoise(self, observations):
        """The auxiliary head's estimate of the clean privileged frame from the (noisy) observation history."""
        if not self.denoiser_hidden_dims:
            raise RuntimeError("this ActorCritic was built without a denoiser head (denoiser_hidden_dims)")
        if self._net is not None and observations.is_cuda:
            return self._net.forward(2, observations.contiguous())
        return self.denoiser(self.obs_normalizer(observations))
