"""Caller-owned buffers of the actor/critic + PPO optimiser and thin call wrappers over the C-ABI."""
import ctypes as C

import torch

from . import _lib as L


SUPPORTED_ACTIVATIONS = "nn.ELU(alpha > 0), nn.SELU(), nn.ReLU(), nn.LeakyReLU(negative_slope >= 0), nn.Tanh(), nn.Sigmoid()"


def activation_spec(activation):
    """(HgymNetConfig.activation, act_alpha, act_scale) of a torch activation module (None: ELU, the reference default).
    Raises NotImplementedError for anything the kernels do not implement; the exact module types are matched, so a subclass
    (which may override forward) is refused too."""
    import torch.nn as nn
    m = activation
    if m is None:
        return L.ACT_ELU, 1.0, 1.0
    t = type(m)
    if t is nn.ELU and m.alpha > 0:
        return L.ACT_ELU, float(m.alpha), 1.0
    if t is nn.SELU:
        return L.ACT_SELU, 1.6732632423543772, 1.0507009873554805
    if t is nn.ReLU:
        return L.ACT_LEAKY_RELU, 0.0, 0.0
    if t is nn.LeakyReLU and m.negative_slope >= 0:
        return L.ACT_LEAKY_RELU, float(m.negative_slope), 0.0
    if t is nn.Tanh:
        return L.ACT_TANH, 0.0, 0.0
    if t is nn.Sigmoid:
        return L.ACT_SIGMOID, 0.0, 0.0
    raise NotImplementedError("activation %r is not implemented by the HIP kernels; supported: %s" % (m, SUPPORTED_ACTIVATIONS))


NOISE_STD_TYPES = ("scalar", "log")


def std_param_spec(noise_std_type):
    """HgymNetConfig.std_param of ActorCritic(noise_std_type=...): "scalar" (the parameter is sigma) or "log" (it is log sigma)."""
    if noise_std_type not in NOISE_STD_TYPES:
        raise ValueError("noise_std_type=%r: must be \"scalar\" or \"log\"" % (noise_std_type,))
    return L.STD_LOG if noise_std_type == "log" else L.STD_SCALAR


def make_net_config(num_obs, num_priv, num_actions, actor_hidden, critic_hidden, precision, max_batch, aux_hidden=None, aux_out=0,
                    aux_target_offset=0, activation=None, fused_activation=False, noise_std_type="scalar"):
    """aux_hidden / aux_out / aux_target_offset: the optional auxiliary (denoising) head obs -> aux_hidden -> aux_out that regresses
    columns [aux_target_offset, aux_target_offset + aux_out) of the privileged row (HgymNetConfig.aux_*).
    activation: the torch module between the Linear layers of every MLP (activation_spec; None: ELU).
    fused_activation: HgymNetConfig.fused_activation -- a bf16 net of the widths the fused kernels take runs them (forward, update tiles,
    bf16 observation shadow) with any activation, not only ELU(1); off by default, because the fused kernels' fast exp2 / rcp forms round
    differently from the layer-by-layer path's libm.  Ignored where the fused kernels are refused anyway; no effect on ELU(1).
    noise_std_type: "scalar" -- the first num_actions parameters are the standard deviations -- or "log" -- they are their logarithms
    (HgymNetConfig.std_param); anything else: ValueError."""
    c = L.NetConfig()
    c.std_param = std_param_spec(noise_std_type)
    c.fused_activation = 1 if fused_activation else 0
    c.activation, c.act_alpha, c.act_scale = activation_spec(activation)
    c.num_obs, c.num_priv, c.num_actions = int(num_obs), int(num_priv), int(num_actions)
    ad = [num_obs] + list(actor_hidden) + [num_actions]
    cd = [num_priv] + list(critic_hidden) + [1]
    c.actor_layers, c.critic_layers = len(ad) - 1, len(cd) - 1
    for i, d in enumerate(ad):
        c.actor_dims[i] = int(d)
    for i, d in enumerate(cd):
        c.critic_dims[i] = int(d)
    c.precision = {"f32": L.F32, "fp32": L.F32, "bf16": L.BF16}[precision] if isinstance(precision, str) else int(precision)
    c.max_batch = int(max_batch)
    if aux_hidden is not None and aux_out > 0:
        xd = [num_obs] + list(aux_hidden) + [int(aux_out)]
        c.aux_layers = len(xd) - 1
        for i, d in enumerate(xd):
            c.aux_dims[i] = int(d)
        c.aux_target_offset = int(aux_target_offset)
    return c


def make_ppo_config(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.001, max_grad_norm=1.0, desired_kl=0.01,
                    adaptive=True, world_size=1, grad_norm_ready=False, aux_coef=0.0, clipped_value_loss=True, mirror_coef=0.0):
    """clipped_value_loss: the reference's use_clipped_value_loss (False: the value loss (R - V)^2, HgymPPOConfig.value_loss_unclipped).
    mirror_coef: weight of the mirror loss (HgymPPOConfig.mirror_coef, rsl_rl's mirror_loss_coeff; 0: off -- make_batch's pair_idx / mirror
    are then ignored)."""
    p = L.PPOConfig()
    p.clip_param, p.value_loss_coef, p.entropy_coef = clip_param, value_loss_coef, entropy_coef
    p.max_grad_norm, p.desired_kl = max_grad_norm, desired_kl
    p.beta1, p.beta2, p.adam_eps = 0.9, 0.999, 1e-8
    p.lr_min, p.lr_max = 1e-5, 1e-2
    p.adaptive_lr = 1 if adaptive else 0
    p.world_size = int(world_size)
    p.aux_coef = float(aux_coef)
    p.grad_norm_ready = 1 if (grad_norm_ready and int(world_size) == 1) else 0    # see HgymPPOConfig
    p.value_loss_unclipped = 0 if clipped_value_loss else 1
    p.mirror_coef = float(mirror_coef)
    return p


class NetBuffers:
    """Flat fp32 master parameters (state_dict order), Adam state, optimiser scalars and the zero-filled
    workspace; exposes per-tensor views named like the reference's ActorCritic.state_dict()."""

    def __init__(self, cfg, device, learning_rate=1e-5, grads_ext=None, obs_norm=None):
        """grads_ext: optional caller-owned (>= P + 1,) fp32 tensor to hold [gradient | KL] (the data-parallel update's direct exchange
        keeps it in peer-mapped memory: dist_utils.P2PComm).
        obs_norm: None (off), or (eps, until) -- empirical observation normalisation folded into the first layer (HgymNet.norm): this
        object owns the block, starts it at mean 0 / var 1 / count 0 and exposes norm_state() / load_norm_state(); until None: the
        statistics never stop.  ValueError for eps < 0 or until < 0."""
        self.cfg = cfg
        self.device = torch.device(device)
        self.P = int(L.lib.hgym_net_param_count(C.byref(cfg)))
        nbytes = int(L.lib.hgym_net_workspace_bytes(C.byref(cfg)))
        if self.P <= 0 or nbytes <= 0:
            raise L.HgymError("bad net config: %s" % L.lib.hgym_last_error().decode())
        z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=self.device)
        self.params, self.adam_m, self.adam_v = z(self.P), z(self.P), z(self.P)
        if grads_ext is not None:
            assert grads_ext.dtype == torch.float32 and grads_ext.is_contiguous() and grads_ext.numel() >= self.P + 1
            grads_ext.zero_()
        self.grads_ext = grads_ext[:self.P + 1] if grads_ext is not None else z(self.P + 1)      # flat gradient + the minibatch KL slot: what the ranks all-reduce, in one piece
        self.grads = self.grads_ext[:self.P]
        self.opt_state = z(L.OPT_STATE, torch.float64)
        self.opt_state[L.OPT_LR] = learning_rate
        self.workspace = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self.workspace.data_ptr()) % 256
        self._ws_ptr = self.workspace.data_ptr() + off
        self.struct = L.Net(L.fptr(self.params), L.fptr(self.grads), L.fptr(self.adam_m), L.fptr(self.adam_v),
                            L.f64ptr(self.opt_state), C.c_void_p(self._ws_ptr))
        self.obs_norm = None
        if obs_norm is not None:
            self.obs_norm = check_obs_norm(*obs_norm)
            self.norm_layout = norm_layout(cfg)
            self._norm_block = torch.zeros(self.norm_layout[L.NORM_BYTES] + 256, dtype=torch.uint8, device=self.device)
            self._norm_off = (-self._norm_block.data_ptr()) % 256
            self.struct.norm = C.c_void_p(self._norm_block.data_ptr() + self._norm_off)
            eps, until = self.obs_norm
            L.check(L.lib.hgym_net_norm_init(C.byref(cfg), C.byref(self.struct), eps, -1 if until is None else until, self.stream()),
                    "hgym_net_norm_init")
        # named views
        self.views = {}
        A = cfg.num_actions
        # the head of the flat vector: sigma ("std") or, with HgymNetConfig.std_param = HGYM_STD_LOG, log sigma ("log_std").  `sigma` is
        # the A standard deviations in both modes: the same memory as "std", or the block of the workspace the library derives
        so = int(L.lib.hgym_net_sigma_offset(C.byref(cfg)))
        if so < -1:
            raise L.HgymError("bad net config: %s" % L.lib.hgym_last_error().decode())
        self.views["log_std" if so >= 0 else "std"] = self.params[:A]
        self.sigma = self.params[:A] if so < 0 else self.workspace[off + so:off + so + 4 * A].view(torch.float32)
        off = A
        nets = [("actor", cfg.actor_dims, cfg.actor_layers), ("critic", cfg.critic_dims, cfg.critic_layers)]
        if cfg.aux_layers > 0:
            nets.append(("denoiser", cfg.aux_dims, cfg.aux_layers))
        for name, dims, n in nets:
            for l in range(n):
                k, o = dims[l], dims[l + 1]
                self.views["%s.%d.weight" % (name, 2 * l)] = self.params[off:off + o * k].view(o, k)
                off += o * k
                self.views["%s.%d.bias" % (name, 2 * l)] = self.params[off:off + o]
                off += o
        assert off == self.P

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream) if self.device.type == "cuda" else None

    def load_state_dict(self, sd):
        for k, v in self.views.items():
            v.copy_(torch.as_tensor(sd[k]).to(self.device).view_as(v))
        self.sync_shadow()

    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.views.items()}

    def grad_views(self):
        out, base = {}, self.params.data_ptr()
        for k, v in self.views.items():
            o = (v.data_ptr() - base) // 4
            out[k] = self.grads[o:o + v.numel()].view_as(v)
        return out

    def sync_shadow(self):
        L.check(L.lib.hgym_net_sync_shadow(C.byref(self.cfg), C.byref(self.struct), self.stream()), "hgym_net_sync_shadow")

    # ------------------------------------------------------------------ observation normalisation (obs_norm)
    def _norm_part(self, slot, count, dtype):
        """A view of `count` elements of `dtype` at layout slot `slot` of the block."""
        if self.obs_norm is None:
            raise RuntimeError("this NetBuffers was built without observation normalisation (obs_norm)")
        o = self._norm_off + int(self.norm_layout[slot])
        if int(self.norm_layout[slot]) < 0:
            raise RuntimeError("the normaliser's block has no part %d for this configuration" % slot)
        return self._norm_block[o:o + count * torch.empty(0, dtype=dtype).element_size()].view(dtype)

    def norm_view(self, name, k=0):
        """Device views into the block: "mean" / "var" (fp64) and "mean_f" / "scale_f" (fp32) of statistics k (0: the actor's, over
        num_obs columns; 1: the critic's, over num_priv), "bias" (fp32, the effective first-layer bias of net k: 0 actor, 1 critic,
        2 auxiliary head), "header" (8 doubles: eps, until, count 0, count 1), "sums" (fp64, what accumulate leaves)."""
        K = (self.cfg.num_obs, self.cfg.num_priv)
        if name in ("mean", "var"):
            return self._norm_part((L.NORM_MEAN if name == "mean" else L.NORM_VAR) + k, K[k], torch.float64)
        if name in ("mean_f", "scale_f"):
            return self._norm_part((L.NORM_MEAN_F if name == "mean_f" else L.NORM_SCALE_F) + k, K[k], torch.float32)
        if name == "bias":
            n1 = (self.cfg.actor_dims[1], self.cfg.critic_dims[1], self.cfg.aux_dims[1])[k]
            return self._norm_part(L.NORM_BIAS + k, n1, torch.float32)
        if name == "header":
            return self._norm_part(L.NORM_HEADER, L.NORM_HEADER_DOUBLES, torch.float64)
        if name == "sums":
            return self._norm_part(L.NORM_SUMS, int(self.norm_layout[L.NORM_SUMS_DOUBLES]), torch.float64)
        raise KeyError(name)

    def norm_accumulate(self, obs, priv):
        """hgym_net_norm_accumulate: the raw fp64 sums (n, sum x, sum x^2 per column) of the M rows of obs (M, num_obs) and priv
        (M, num_priv), contiguous fp32, into the block's sums part (overwritten)."""
        assert obs.is_contiguous() and priv.is_contiguous() and obs.dtype == torch.float32 and priv.dtype == torch.float32
        assert obs.shape[0] == priv.shape[0] and obs.shape[1] == self.cfg.num_obs and priv.shape[1] == self.cfg.num_priv
        L.check(L.lib.hgym_net_norm_accumulate(C.byref(self.cfg), C.byref(self.struct), L.fptr(obs), L.fptr(priv), int(obs.shape[0]),
                                               self.stream()), "hgym_net_norm_accumulate")

    def norm_merge(self):
        """hgym_net_norm_merge: the sums part merged into the running statistics, then the refold."""
        L.check(L.lib.hgym_net_norm_merge(C.byref(self.cfg), C.byref(self.struct), self.stream()), "hgym_net_norm_merge")

    def norm_unfold_grad(self):
        """hgym_net_norm_unfold_grad: call between ppo_grad and the exchange / ppo_apply."""
        L.check(L.lib.hgym_net_norm_unfold_grad(C.byref(self.cfg), C.byref(self.struct), self.stream()), "hgym_net_norm_unfold_grad")

    def norm_state(self):
        """{"obs": {...}, "critic_obs": {...}}, each mean, var (fp64 clones), count, eps, until -- what a checkpoint carries."""
        h = self.norm_view("header")
        eps, until = self.obs_norm
        return {name: dict(mean=self.norm_view("mean", k).clone(), var=self.norm_view("var", k).clone(), count=h[2 + k].clone(),
                           eps=eps, until=until) for k, name in enumerate(("obs", "critic_obs"))}

    def load_norm_state(self, state):
        """The inverse of norm_state() -- mean, var, count of both statistics (eps and until are this object's own) -- then the refold."""
        h = self.norm_view("header")
        for k, name in enumerate(("obs", "critic_obs")):
            st = state[name]
            for part in ("mean", "var"):
                v = self.norm_view(part, k)
                v.copy_(torch.as_tensor(st[part], dtype=torch.float64).to(self.device).view_as(v))
            h[2 + k:3 + k] = torch.as_tensor(st["count"], dtype=torch.float64).to(self.device).reshape(1)
        self.norm_sums_clear()
        self.norm_merge()       # an empty batch: nothing merges, the floats and the fold are recomputed from the loaded state

    def norm_sums_clear(self):
        self.norm_view("sums").zero_()

    def forward(self, which, x):
        M = x.shape[0]
        nout = self.cfg.num_actions if which == 0 else (1 if which == 1 else self.cfg.aux_dims[self.cfg.aux_layers])
        y = torch.empty(M, nout, device=self.device)
        L.check(L.lib.hgym_mlp_forward(C.byref(self.cfg), C.byref(self.struct), which, M, L.fptr(x), x.stride(0), L.fptr(y),
                                       self.stream()), "hgym_mlp_forward")
        return y

    def shadow_ld(self, which):
        """Leading dimension (elements) of the bf16 shadow of the actor's (0) / critic's (1) input rows; 0: no shadow on this path."""
        return int(L.lib.hgym_net_shadow_ld(C.byref(self.cfg), int(which)))

    def shadow_struct(self, obs_bf16, priv_bf16):
        """HgymObsShadow over two (M, ld) torch.bfloat16 tensors (the caller keeps them alive); either may be None (that member is
        not written by the launch)."""
        for t in (obs_bf16, priv_bf16):
            assert t is None or (t.dtype == torch.bfloat16 and t.is_contiguous())
        p = lambda t: (None, 0) if t is None else (C.c_void_p(t.data_ptr()), t.shape[-1])
        return L.ObsShadow(*p(obs_bf16), *p(priv_bf16))

    def critic_values(self, priv, values, priv_bf16=None):
        """hgym_critic_values: V of every row of `priv` ((M, num_priv) fp32, contiguous) into `values` ((M,) or (M, 1) fp32); priv_bf16:
        optional (M, ld) bfloat16 shadow rows to fill.  M may exceed the configuration's max_batch."""
        assert priv.is_contiguous() and values.is_contiguous() and priv.dtype == torch.float32 and values.numel() == priv.shape[0]
        sh = None if priv_bf16 is None else C.byref(self.shadow_struct(None, priv_bf16))
        L.check(L.lib.hgym_critic_values(C.byref(self.cfg), C.byref(self.struct), int(priv.shape[0]), L.fptr(priv), L.fptr(values), sh,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hgym_critic_values")

    def act(self, obs, priv, z=None, seed=0, step_counter=None, out=None, env_fin=None, shadow=None):
        """env_fin: optional (HgymEnvConfig, HgymEnvState, HgymEnvOut) of an env step whose finaliser was postponed
        (HgymEnvOut.defer_finalize): it runs as one extra workgroup of this launch (hgym_policy_act_fin).
        shadow: optional (obs_bf16, priv_bf16) tensors receiving the bf16 of the rows read (HgymObsShadow)."""
        sh = None if shadow is None else C.byref(self.shadow_struct(*shadow))
        M = obs.shape[0]
        A = self.cfg.num_actions
        if out is None:
            e = lambda *s: torch.empty(*s, device=self.device)
            out = dict(actions=e(M, A), mu=e(M, A), sigma=e(M, A), logp=e(M), values=e(M, 1))
        if env_fin is not None:
            ecfg, est, eout = env_fin
            L.check(L.lib.hgym_policy_act_fin(C.byref(self.cfg), C.byref(self.struct), M, L.fptr(obs), L.fptr(priv), L.fptr(z), int(seed),
                                              L.i64ptr(step_counter), L.fptr(out["actions"]), L.fptr(out["mu"]), L.fptr(out["sigma"]),
                                              L.fptr(out["logp"]), L.fptr(out["values"]), C.byref(ecfg), C.byref(est), C.byref(eout), sh,
                                              self.stream()), "hgym_policy_act_fin")
            return out
        L.check(L.lib.hgym_policy_act(C.byref(self.cfg), C.byref(self.struct), M, L.fptr(obs), L.fptr(priv), L.fptr(z), int(seed),
                                      L.i64ptr(step_counter), L.fptr(out["actions"]), L.fptr(out["mu"]), L.fptr(out["sigma"]),
                                      L.fptr(out["logp"]), L.fptr(out["values"]), sh, self.stream()), "hgym_policy_act")
        return out

    def ppo_diagnostics(self, ppo, cols, out_block):
        """hgym_ppo_diagnostics over the rows of `cols` -- the nine flattened storage columns in make_batch's order (obs, priv, actions,
        values, advantages, returns, logp, mu, sigma), contiguous fp32, any number M of rows -- with the parameters as they are now:
        hgym_ppo_diag_reset, the two forwards piece by piece, the reduction.  out_block: L.diag_block(M, device) of the caller; it
        holds the sums afterwards in stream order (diag_from_block reads them).  Nothing is read back, nothing allocated after the
        first call (the forwards' scratch, max_batch x 13 floats, is kept)."""
        M = int(cols[0].shape[0])
        for t in cols:
            assert t.is_contiguous() and t.dtype == torch.float32 and t.shape[0] == M
        assert out_block.dtype == torch.float64 and out_block.is_contiguous() and out_block.numel() >= L.diag_block_doubles(M)
        if getattr(self, "_diag_scratch", None) is None:
            self._diag_scratch = torch.empty(int(self.cfg.max_batch) * 13, dtype=torch.float32, device=self.device)
        rows = L.Batch(*[L.fptr(t) for t in cols], None, 0, None, None, M)
        L.check(L.lib.hgym_ppo_diag_reset(M, L.f64ptr(out_block), self.stream()), "hgym_ppo_diag_reset")
        L.check(L.lib.hgym_ppo_diagnostics(C.byref(self.cfg), C.byref(ppo), C.byref(self.struct), C.byref(rows), M, L.fptr(self._diag_scratch),
                                           L.f64ptr(out_block), self.stream()), "hgym_ppo_diagnostics")
        return out_block

    def ppo_grad(self, ppo, batch):
        L.check(L.lib.hgym_ppo_grad(C.byref(self.cfg), C.byref(ppo), C.byref(self.struct), C.byref(batch), self.stream()), "hgym_ppo_grad")

    def ppo_grad_smooth(self, ppo, batch, smooth):
        """hgym_ppo_grad_smooth: hgym_ppo_grad with the smoothness regulariser (make_smooth); both coefficients 0: hgym_ppo_grad itself."""
        L.check(L.lib.hgym_ppo_grad_smooth(C.byref(self.cfg), C.byref(ppo), C.byref(self.struct), C.byref(batch), C.byref(smooth), self.stream()),
                "hgym_ppo_grad_smooth")

    def ppo_grad_smooth_mirror(self, ppo, batch, smooth, head_partials):
        """hgym_ppo_grad_smooth_mirror: hgym_ppo_grad with the mirror loss (ppo.mirror_coef, make_batch's mirror fields) and the smoothness
        regulariser (make_smooth) in one actor head.  head_partials: float32 device scratch of at least smooth_mirror_partials(batch.B)
        elements, 16-byte aligned, that the caller keeps alive.  mirror_coef 0: hgym_ppo_grad_smooth; both coefficients 0: hgym_ppo_grad."""
        assert head_partials is None or (head_partials.dtype == torch.float32 and head_partials.is_contiguous())
        L.check(L.lib.hgym_ppo_grad_smooth_mirror(C.byref(self.cfg), C.byref(ppo), C.byref(self.struct), C.byref(batch), C.byref(smooth),
                                                  L.fptr(head_partials), 0 if head_partials is None else int(head_partials.numel()),
                                                  self.stream()), "hgym_ppo_grad_smooth_mirror")

    def ppo_grad_guide(self, ppo, batch, guide):
        """hgym_ppo_grad_guide: hgym_ppo_grad with a frozen teacher's cloning term (make_guide) in the actor's head.  The coefficient is read
        from the device on every call, so a captured call follows hgym.guide_schedule.  Refused: ppo.mirror_coef > 0, several ranks."""
        L.check(L.lib.hgym_ppo_grad_guide(C.byref(self.cfg), C.byref(ppo), C.byref(self.struct), C.byref(batch), C.byref(guide), self.stream()),
                "hgym_ppo_grad_guide")

    def ppo_grad_part(self, ppo, batch, part):
        """hgym_ppo_grad in two halves (data-parallel update): after part 0 `grads_ext[:bucket_split]` (std | actor, the larger
        bucket) is final, after part 1 `grads_ext[bucket_split:]` (critic | auxiliary head | KL slot)."""
        L.check(L.lib.hgym_ppo_grad_part(C.byref(self.cfg), C.byref(ppo), C.byref(self.struct), C.byref(batch), int(part), self.stream()),
                "hgym_ppo_grad_part")

    def bc_grad(self, bc, batch, target, sums):
        """hgym_bc_grad: one behaviour-cloning minibatch of the actor (make_bc_config, make_bc_batch).  target: (rows, num_actions) fp32,
        contiguous, gathered through the batch's idx; sums: float64 (2,), [0] += the minibatch's loss, [1] += 1."""
        assert target.dtype == torch.float32 and target.is_contiguous() and sums.dtype == torch.float64 and sums.numel() >= 2
        L.check(L.lib.hgym_bc_grad(C.byref(self.cfg), C.byref(bc), C.byref(self.struct), C.byref(batch), L.fptr(target), L.f64ptr(sums),
                                   self.stream()), "hgym_bc_grad")

    def vf_grad(self, vf, batch, sums):
        """hgym_vf_grad: one critic-only minibatch (make_vf_config, make_vf_batch).  sums: float64 (2,), [0] += the minibatch's mean value
        loss (unweighted), [1] += 1.  The step is ppo_apply's with adaptive_lr = 0 and grad_norm_ready = 0."""
        assert sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() >= 2
        L.check(L.lib.hgym_vf_grad(C.byref(self.cfg), C.byref(vf), C.byref(self.struct), C.byref(batch), L.f64ptr(sums), self.stream()),
                "hgym_vf_grad")

    def bc_vf_grad(self, bc, vf, batch, target, bc_sums, vf_sums):
        """hgym_bc_vf_grad: one cloning minibatch that also trains the critic -- bit for bit bc_grad followed by vf_grad with
        keep_others = 1, in fewer launches.  batch: make_vf_batch with obs; target, bc_sums as for bc_grad; vf_sums as for vf_grad."""
        assert target.dtype == torch.float32 and target.is_contiguous()
        for t in (bc_sums, vf_sums):
            assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() >= 2
        L.check(L.lib.hgym_bc_vf_grad(C.byref(self.cfg), C.byref(bc), C.byref(vf), C.byref(self.struct), C.byref(batch), L.fptr(target),
                                      L.f64ptr(bc_sums), L.f64ptr(vf_sums), self.stream()), "hgym_bc_vf_grad")

    @property
    def bucket_split(self):
        """Offset of the critic's first parameter in the flat vector: the boundary of the two gradient buckets."""
        return int(L.lib.hgym_net_param_offset(C.byref(self.cfg), 1))

    def ppo_apply(self, ppo):
        L.check(L.lib.hgym_ppo_apply(C.byref(self.cfg), C.byref(ppo), C.byref(self.struct), self.stream()), "hgym_ppo_apply")


def check_obs_norm(eps, until):
    """(float eps, int until or None) of an obs_norm=(eps, until) argument; ValueError for eps < 0 / not finite or until < 0."""
    import math
    eps = float(eps)
    if not (eps >= 0.0 and math.isfinite(eps)):
        raise ValueError("normalization_eps=%r: must be finite and >= 0" % (eps,))
    if until is not None:
        if int(until) != until or until < 0:
            raise ValueError("normalization_until=%r: must be None or an integer row count >= 0" % (until,))
        until = int(until)
    return eps, until


def norm_layout(cfg):
    """hgym_net_norm_layout: the list of HGYM_NORM_LAYOUT numbers (L.NORM_*) for a net config; needs no device."""
    out = (C.c_int64 * L.NORM_LAYOUT)()
    L.check(L.lib.hgym_net_norm_layout(C.byref(cfg), out), "hgym_net_norm_layout")
    return list(out)


def make_batch(obs, priv, actions, values, advantages, returns, logp, mu, sigma, idx, obs_bf16=None, priv_bf16=None, pair_idx=None, mirror=None):
    """All (T*N, *) flattened, contiguous fp32; idx int64 (B,).  obs_bf16 / priv_bf16: optional (T*N, ld) bfloat16 shadows of obs /
    priv (ld = NetBuffers.shadow_ld), both or neither.
    The mirror loss (make_ppo_config(mirror_coef > 0); both or neither): pair_idx int64 (B,), the storage row holding the mirrored observation
    of every row of idx; mirror = (act_src int32 (A,), act_sign fp32 (A,), target fp32 scratch of at least B * A elements, 16-byte aligned,
    sums float64 (2,)) -- device tensors the caller keeps alive; sums[0] += the minibatch's MSE, sums[1] += 1."""
    for t in (obs, priv, actions, values, advantages, returns, logp, mu, sigma):
        assert t.is_contiguous() and t.dtype == torch.float32
    assert idx.dtype == torch.int64 and idx.is_contiguous()
    assert (obs_bf16 is None) == (priv_bf16 is None)
    sb = (None, None)
    if obs_bf16 is not None:
        assert obs_bf16.dtype == torch.bfloat16 and priv_bf16.dtype == torch.bfloat16 and obs_bf16.is_contiguous() and priv_bf16.is_contiguous()
        assert obs_bf16.shape[0] == obs.shape[0] and priv_bf16.shape[0] == priv.shape[0]
        sb = (C.c_void_p(obs_bf16.data_ptr()), C.c_void_p(priv_bf16.data_ptr()))
    b = L.Batch(L.fptr(obs), L.fptr(priv), L.fptr(actions), L.fptr(values), L.fptr(advantages), L.fptr(returns), L.fptr(logp),
                L.fptr(mu), L.fptr(sigma), L.i64ptr(idx), int(idx.numel()), sb[0], sb[1], int(obs.shape[0]))
    assert (pair_idx is None) == (mirror is None)
    if mirror is not None:
        src, sign, target, sums = mirror
        A = int(actions.shape[1])
        assert pair_idx.dtype == torch.int64 and pair_idx.is_contiguous() and pair_idx.numel() == idx.numel()
        assert src.dtype == torch.int32 and sign.dtype == torch.float32 and src.numel() == A and sign.numel() == A
        assert src.is_contiguous() and sign.is_contiguous()
        assert target.dtype == torch.float32 and target.is_contiguous() and target.numel() >= idx.numel() * A
        assert sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() >= 2
        b.pair_idx, b.mirror_act_src, b.mirror_act_sign = L.i64ptr(pair_idx), C.cast(src.data_ptr(), C.POINTER(C.c_int32)), L.fptr(sign)
        b.mirror_target, b.mirror_sums = L.fptr(target), L.f64ptr(sums)
    return b


def smooth_ld(num_obs):
    """Leading dimension (floats) of HgymSmooth.rows: the observation width rounded up to 4, so that every row starts on 16 bytes."""
    return (int(num_obs) + 3) // 4 * 4


def smooth_mirror_partials(mb):
    """Length (floats) of hgym_ppo_grad_smooth_mirror's head_partials for minibatches of mb rows: 4 per tile of 64 rows."""
    return 4 * ((int(mb) + 63) // 64)


def make_smooth(temporal_coef=0.0, spatial_coef=0.0, next_idx=None, next_weight=None, noise_std=None, seed=0, target_next=None,
                target_near=None, rows=None, sums=None):
    """HgymSmooth of hgym_ppo_grad_smooth.  Coefficients: finite and >= 0 (ValueError otherwise); a term at 0 is off and its tensors may be
    None.  Device tensors the caller keeps alive: next_idx int64 (B,), next_weight fp32 (B,) (hgym.smooth_pairs writes both); noise_std fp32
    (num_obs,); target_next / target_near fp32 scratch of at least B * num_actions elements; rows fp32 scratch of at least B *
    smooth_ld(num_obs) elements; sums float64 (4,), zeroed by the caller.  Scratch must be 16-byte aligned (the library refuses otherwise)."""
    import math
    lt, ls = float(temporal_coef), float(spatial_coef)
    for name, v in (("temporal_coef", lt), ("spatial_coef", ls)):
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError("%s=%r: must be finite and >= 0" % (name, v))
    for t, dt in ((next_idx, torch.int64), (next_weight, torch.float32), (noise_std, torch.float32), (target_next, torch.float32),
                  (target_near, torch.float32), (rows, torch.float32), (sums, torch.float64)):
        assert t is None or (t.dtype == dt and t.is_contiguous())
    assert sums is None or sums.numel() >= 4
    return L.Smooth(lt, ls, L.i64ptr(next_idx), L.fptr(next_weight), L.fptr(noise_std), int(seed) & 0xFFFFFFFFFFFFFFFF, L.fptr(target_next),
                    L.fptr(target_near), L.fptr(rows), L.f64ptr(sums))


GUIDE_MODES = ("constant", "step", "linear")


def make_guide_schedule(mode="constant", coef=0.0, final_value=None, initial_step=0, final_step=0):
    """HgymGuideSchedule of hgym_guide_schedule.  mode: "constant", "step" (coef while k < final_step, then final_value) or "linear" (coef
    up to initial_step, a straight line to final_value at final_step, final_value beyond).  ValueError for an unknown mode, a coefficient
    that is not finite and >= 0, a negative step, or linear with final_step <= initial_step."""
    import math
    if mode not in GUIDE_MODES:
        raise ValueError("mode=%r: one of %s" % (mode, ", ".join(GUIDE_MODES)))
    c = float(coef)
    f = c if final_value is None or mode == "constant" else float(final_value)
    for name, v in (("coef", c), ("final_value", f)):
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError("%s=%r: must be finite and >= 0" % (name, v))
    i0, i1 = (0, 0) if mode == "constant" else (int(initial_step) if mode == "linear" else 0, int(final_step))
    if i0 < 0 or i1 < 0:
        raise ValueError("initial_step=%r / final_step=%r: must be >= 0" % (initial_step, final_step))
    if mode == "linear" and i1 <= i0:
        raise ValueError("final_step=%d must be greater than initial_step=%d" % (i1, i0))
    return L.GuideSchedule(c, f, i0, i1, GUIDE_MODES.index(mode), 0)


def guide_schedule_coef(sched, k):
    """The coefficient hgym_guide_schedule writes at update count k, bit for bit: python doubles, left to right, rounded to fp32 once.
    sched: an HgymGuideSchedule (make_guide_schedule).  Returns the fp32 value as a python float."""
    import struct
    k = int(k)
    c, f, i0, i1 = float(sched.coef), float(sched.final_value), int(sched.initial_step), int(sched.final_step)
    if sched.mode == L.GUIDE_STEP:
        v = c if k < i1 else f
    elif sched.mode == L.GUIDE_LINEAR:
        if k <= i0:
            v = c
        elif k >= i1:
            v = f
        else:
            v = c + (f - c) * float(k - i0) / float(i1 - i0)
    else:
        v = c
    return struct.unpack("f", struct.pack("f", v))[0]


def guide_schedule(sched, count, coef, stream=None):
    """hgym_guide_schedule on the current stream: coef[0] = schedule(count[0]) as fp32, then count[0] += 1.  count: int64 (1,) device tensor,
    coef: float32 (1,) device tensor; one launch with fixed arguments, capturable."""
    assert count.dtype == torch.int64 and count.numel() >= 1 and coef.dtype == torch.float32 and coef.numel() >= 1
    assert count.is_cuda and coef.is_cuda
    s = C.c_void_p(torch.cuda.current_stream(count.device).cuda_stream) if stream is None else stream
    L.check(L.lib.hgym_guide_schedule(C.byref(sched), L.i64ptr(count), L.fptr(coef), s), "hgym_guide_schedule")


def make_guide(teacher_mu, coef, sums):
    """HgymGuide of hgym_ppo_grad_guide.  Device tensors the caller keeps alive: teacher_mu fp32 (num_rows, num_actions) contiguous, 16-byte
    aligned -- the frozen teacher's mean of every stored row, gathered through the batch's idx; coef fp32 (1,), this update's coefficient
    (hgym.guide_schedule writes it); sums float64 (2,), zeroed by the caller: [0] += the minibatch's unweighted MSE, [1] += 1."""
    assert teacher_mu.dtype == torch.float32 and teacher_mu.is_contiguous() and teacher_mu.dim() == 2
    assert coef.dtype == torch.float32 and coef.numel() >= 1 and sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() >= 2
    return L.Guide(L.fptr(teacher_mu), L.fptr(coef), L.f64ptr(sums))


BC_LOSS_TYPES = ("mse", "huber")


def make_bc_config(loss_type="mse", huber_delta=1.0):
    """HgymBCConfig of hgym_bc_grad: loss_type "mse" (torch's mse_loss) or "huber" (torch's huber_loss with delta = huber_delta > 0, finite).
    ValueError for anything else."""
    import math
    if loss_type not in BC_LOSS_TYPES:
        raise ValueError("loss_type=%r: one of %s" % (loss_type, ", ".join(BC_LOSS_TYPES)))
    d = float(huber_delta)
    if loss_type == "huber" and not (d > 0.0 and math.isfinite(d)):
        raise ValueError("huber_delta=%r: must be finite and > 0" % (huber_delta,))
    return L.BCConfig(L.BC_HUBER if loss_type == "huber" else L.BC_MSE, d)


def make_bc_batch(obs, idx, obs_bf16=None):
    """The HgymBatch hgym_bc_grad reads: obs (rows, num_obs) fp32 contiguous, idx int64 (B,), optionally the (rows, ld) bfloat16 shadow of
    obs.  Every other member stays NULL."""
    assert obs.is_contiguous() and obs.dtype == torch.float32 and idx.dtype == torch.int64 and idx.is_contiguous()
    b = L.Batch()
    b.obs, b.idx, b.B, b.num_rows = L.fptr(obs), L.i64ptr(idx), int(idx.numel()), int(obs.shape[0])
    if obs_bf16 is not None:
        assert obs_bf16.dtype == torch.bfloat16 and obs_bf16.is_contiguous() and obs_bf16.shape[0] == obs.shape[0]
        b.obs_bf16 = C.c_void_p(obs_bf16.data_ptr())
    return b


def make_vf_config(clip_param=0.2, value_coef=1.0, clipped_value_loss=True, keep_others=False):
    """HgymVFConfig of hgym_vf_grad / hgym_bc_vf_grad.  clip_param: the value clip range (finite and >= 0; not read by the unclipped
    form); value_coef: multiplies the gradient, not the reported loss (finite and >= 0); clipped_value_loss: the reference's
    use_clipped_value_loss; keep_others: leave the gradient outside the critic's region as found and ADD the critic's squared norm
    (False: that region becomes +0.0 and the norm is the critic's alone).  ValueError for anything else."""
    import math
    c, k = float(clip_param), float(value_coef)
    if clipped_value_loss and not (c >= 0.0 and math.isfinite(c)):
        raise ValueError("clip_param=%r: must be finite and >= 0" % (clip_param,))
    if not (k >= 0.0 and math.isfinite(k)):
        raise ValueError("value_coef=%r: must be finite and >= 0" % (value_coef,))
    return L.VFConfig(c if clipped_value_loss else 0.0, k, 0 if clipped_value_loss else 1, 1 if keep_others else 0)


def make_vf_batch(priv, values, returns, idx, priv_bf16=None, obs=None, obs_bf16=None):
    """The HgymBatch hgym_vf_grad reads: priv (rows, num_priv), values (rows,) -- None with the unclipped loss -- and returns (rows,),
    fp32 contiguous; idx int64 (B,); optionally the (rows, ld) bfloat16 shadow of priv.  obs / obs_bf16: what hgym_bc_vf_grad reads beside
    them (make_bc_batch's).  Every other member stays NULL."""
    for t in (priv, values, returns, obs):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32)
    assert idx.dtype == torch.int64 and idx.is_contiguous()
    rows = int(priv.shape[0])
    assert returns.numel() == rows and (values is None or values.numel() == rows) and (obs is None or obs.shape[0] == rows)
    b = L.Batch()
    b.priv, b.values, b.returns = L.fptr(priv), L.fptr(values), L.fptr(returns)
    b.idx, b.B, b.num_rows = L.i64ptr(idx), int(idx.numel()), rows
    if obs is not None:
        b.obs = L.fptr(obs)
    for name, t in (("priv_bf16", priv_bf16), ("obs_bf16", obs_bf16)):
        if t is not None:
            assert t.dtype == torch.bfloat16 and t.is_contiguous() and t.shape[0] == rows
            setattr(b, name, C.c_void_p(t.data_ptr()))
    return b


DIAG_KEYS = ("samples", "clip_fraction", "kl", "approx_kl", "ratio_mean", "ratio_max", "ratio_min", "surrogate", "entropy",
             "value_clip_fraction", "return_mean", "return_std", "explained_variance", "explained_variance_new", "value_rmse",
             "value_rmse_new")


def diag_from_block(block, clip_param=None):
    """The sums of a diagnostics block (hgym_ppo_diag_reduce's totals, block[:HGYM_DIAG_SUMS]: a tensor, or any sequence of 16 numbers)
    -> a dict of python floats, DIAG_KEYS:
      samples (int), clip_fraction (rows whose ratio left [1 - clip, 1 + clip]), kl (mean analytic KL(old || new)), approx_kl (mean of
      ratio - 1 - log ratio), ratio_mean / ratio_max / ratio_min, surrogate (the clipped surrogate loss over the whole batch), entropy,
      value_clip_fraction (rows with |V_new - V_old| > clip), return_mean / return_std (population), explained_variance = 1 -
      Var(R - V_old) / Var(R) for the critic that collected the data and explained_variance_new for the updated one, value_rmse /
      value_rmse_new = sqrt(mean (R - V)^2).
    Var(R) == 0: nan for both explained variances; samples == 0: nan for everything but samples.  Pure host arithmetic in python
    doubles.  clip_param is not needed (the counts were taken on the device); accepted so that callers may pass what they ran with."""
    import math
    b = [float(x) for x in (block[:L.DIAG_SUMS].tolist() if hasattr(block, "tolist") else list(block)[:L.DIAG_SUMS])]
    n = b[L.DIAG_COUNT]
    nan = float("nan")
    if n <= 0:
        return dict({k: nan for k in DIAG_KEYS}, samples=0)
    mean = lambda i: b[i] / n
    var = lambda i, i2: max(b[i2] / n - (b[i] / n) ** 2, 0.0)
    var_r = var(L.DIAG_RET, L.DIAG_RET_SQ)
    ev = lambda i, i2: (1.0 - var(i, i2) / var_r) if var_r > 0.0 else nan
    return dict(samples=int(n), clip_fraction=mean(L.DIAG_CLIPPED), kl=mean(L.DIAG_KL), approx_kl=mean(L.DIAG_APPROX_KL),
                ratio_mean=mean(L.DIAG_RATIO), ratio_max=b[L.DIAG_RATIO_MAX], ratio_min=b[L.DIAG_RATIO_MIN], surrogate=mean(L.DIAG_SURROGATE),
                entropy=mean(L.DIAG_ENTROPY), value_clip_fraction=mean(L.DIAG_VALUE_CLIPPED), return_mean=mean(L.DIAG_RET),
                return_std=math.sqrt(var_r), explained_variance=ev(L.DIAG_ERR_OLD, L.DIAG_ERR_OLD_SQ),
                explained_variance_new=ev(L.DIAG_ERR_NEW, L.DIAG_ERR_NEW_SQ), value_rmse=math.sqrt(mean(L.DIAG_ERR_OLD_SQ)),
                value_rmse_new=math.sqrt(mean(L.DIAG_ERR_NEW_SQ)))


def opt_summary(o, aux):
    """What a log block takes from an opt_state snapshot (a tensor, or any sequence of HGYM_OPT_STATE numbers) after an update: the per-update
    sums over the minibatches they were taken on (at least 1).  aux: the auxiliary head is trained (else denoise_loss is None)."""
    n = max(float(o[L.OPT_MINIBATCHES]), 1.0)
    return dict(mean_value_loss=float(o[L.OPT_VALUE_SUM]) / n, mean_surrogate_loss=float(o[L.OPT_SURROGATE_SUM]) / n,
                denoise_loss=float(o[L.OPT_AUX_SUM]) / n if aux else None, learning_rate=float(o[L.OPT_LR]))
