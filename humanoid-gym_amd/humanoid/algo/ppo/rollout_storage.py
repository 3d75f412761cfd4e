"""Time-major rollout buffer with the reference's fields and methods (algo/ppo/rollout_storage.py:36-182).

Observation buffers carry ONE extra time slot: the env writes the observations of step t+1 directly into slot
t+1 (LeggedRobot.bind_outputs), so nothing is copied per step; slot T holds the bootstrap observation and is
rotated to slot 0 when the buffer is cleared.  `observations` / `privileged_observations` are the (T, N, .) views.
GAE and advantage normalisation run in libhgym_hip.so (wavefront scan)."""
import ctypes as C

import torch


def mirror_pair_rows(idx, T, N):
    """The partner of every row of `idx` in the (2 T + 1)-slot layout of RolloutStorage.enable_mirror: the row that holds the mirrored
    observation of the same transition.  Original row r < T N <-> mirrored row (T + 1) N + r; an involution on those rows; the bootstrap
    slot (rows [T N, (T + 1) N)) is never named for a row outside it.  A pure function: device operations with fixed arguments, no host
    read -- capturable."""
    off = (int(T) + 1) * int(N)
    return torch.where(idx < int(T) * int(N), idx + off, idx - off)


class RolloutStorage:
    class Transition:
        def __init__(self):
            self.observations = None
            self.critic_observations = None
            self.actions = None
            self.rewards = None
            self.dones = None
            self.values = None
            self.actions_log_prob = None
            self.action_mean = None
            self.action_sigma = None
            self.hidden_states = None

        def clear(self):
            self.__init__()

    def __init__(self, num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, actions_shape, device="cpu"):
        self.device = device
        self.obs_shape, self.privileged_obs_shape, self.actions_shape = obs_shape, privileged_obs_shape, actions_shape
        T, N = num_transitions_per_env, num_envs
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=self.device)
        self._obs_all = z(T + 1, N, *obs_shape)
        self.observations = self._obs_all[:T]
        if privileged_obs_shape[0] is not None:
            self._priv_all = z(T + 1, N, *privileged_obs_shape)
            self.privileged_observations = self._priv_all[:T]
        else:
            self._priv_all = None
            self.privileged_observations = None
        self.rewards = z(T, N, 1)
        self.actions = z(T, N, *actions_shape)
        self.dones = z(T, N, 1, dtype=torch.uint8)
        self.actions_log_prob = z(T, N, 1)
        self.values = z(T, N, 1)
        self.returns = z(T, N, 1)
        self.advantages = z(T, N, 1)
        self.mu = z(T, N, *actions_shape)
        self.sigma = z(T, N, *actions_shape)
        self.num_transitions_per_env, self.num_envs = T, N
        self.saved_hidden_states_a = self.saved_hidden_states_c = None
        self._stats = z(4 + 2 * ((N + 15) // 16), dtype=torch.float64)      # HGYM_GAE_STATS_DOUBLES(N): [sum, sum of squares, count | counter, partials]
        self.step = 0
        # optional bf16 shadows of the two observation buffers (enable_shadow): written by the policy launch that reads the slot,
        # read by the update instead of the fp32 rows
        self._obs_bf16 = self._priv_bf16 = None
        self.shadow_valid = [False] * T
        # deferred values (enable_deferred_values): the bootstrap flags of every step + the value of the bootstrap observation
        self.time_outs = self.last_values = None
        # left-right mirrored half (enable_mirror): the device tables, None without it
        self._mirror = None
        # per-minibatch advantage normalisation (enable_minibatch_advantages): the second advantages column, None without it
        self.advantages_mb = self._adv_mb_scratch = None

    def enable_minibatch_advantages(self, segments, seg_len):
        """Native extension (PPO.advantage_normalization = "minibatch"): `advantages_mb`, a second advantages column laid out like the one
        batch_columns() names (T N rows, or (2 T + 1) N with enable_mirror -- call this after it), zero-filled once, and the scratch of
        hgym_adv_normalize_minibatches for `segments` minibatches of `seg_len` rows."""
        from hgym import _lib as L
        rows = (self.num_transitions_per_env if self._mirror is None else 2 * self.num_transitions_per_env + 1) * self.num_envs
        self.advantages_mb = torch.zeros(rows, dtype=torch.float32, device=self.device)
        self._adv_mb_scratch = L.adv_mb_scratch(segments, seg_len, self.device)

    def normalize_minibatch_advantages(self, perm, segments):
        """advantages_mb[perm[j]] = the advantage of row perm[j] standardised by the mean and unbiased deviation of its minibatch
        perm[s * mb:(s + 1) * mb] (hgym_adv_normalize_minibatches: one pass, two launches, fixed arguments -- capturable).  perm: distinct
        rows of the column batch_columns() names (after mirror_index).  Rows perm does not name keep their 0.  -> advantages_mb."""
        import hgym
        adv = self.advantages.view(-1) if self._mirror is None else self._col_store["advantages"].view(-1)
        hgym.adv_normalize_minibatches(perm, adv, self.advantages_mb, segments, self._adv_mb_scratch)
        return self.advantages_mb

    def minibatch_advantages_key(self):
        """PPO.update_graph_key's entry: the column and the scratch the per-minibatch pass names; None without them."""
        return None if self.advantages_mb is None else (self.advantages_mb.data_ptr(), self._adv_mb_scratch.data_ptr())

    def enable_rnd(self, num_states, num_outputs):
        """Native extension (PPO.rnd): rnd_states (T + 1, N, S) -- a contiguous copy of the chosen observation columns of slots 0 .. T (the
        net kernels gather rows without a leading dimension) --, rnd_target (T + 1, N, K), rnd_pred (T, N, K) -- the predictor over slots
        1 .. T --, rnd_error and rnd_intrinsic (T, N).  Filled by RandomNetworkDistillation.reward_pass."""
        T, N = self.num_transitions_per_env, self.num_envs
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)
        self.rnd_states, self.rnd_target = z(T + 1, N, int(num_states)), z(T + 1, N, int(num_outputs))
        self.rnd_pred, self.rnd_error, self.rnd_intrinsic = z(T, N, int(num_outputs)), z(T, N), z(T, N)

    def enable_guidance(self, num_actions):
        """Native extension (PPO.guidance): teacher_mu (T + 1, N, A) -- the frozen teacher's mean of every stored observation row, one row
        per row of the observation column (slot T's are never read); filled by Guidance.teacher_pass at the end of compute_returns."""
        T, N = self.num_transitions_per_env, self.num_envs
        self.teacher_mu = torch.zeros(T + 1, N, int(num_actions), dtype=torch.float32, device=self.device)

    def enable_shadow(self, ld_obs, ld_priv):
        """Native extension: allocate (T, N, ld) bfloat16 copies of `observations` / `privileged_observations` (ld = the widths
        padded to 128, zero pad columns).  Slot s counts as valid once a policy launch has written it (shadow_slot)."""
        if self._priv_all is None or ld_obs <= 0 or ld_priv <= 0:
            return False
        T, N = self.num_transitions_per_env, self.num_envs
        slots = T if self._mirror is None else 2 * T + 1       # (enable_mirror: the same slot layout as every mirrored column)
        self._obs_bf16_store = torch.zeros(slots, N, int(ld_obs), dtype=torch.bfloat16, device=self.device)
        self._priv_bf16_store = torch.zeros(slots, N, int(ld_priv), dtype=torch.bfloat16, device=self.device)
        self._obs_bf16, self._priv_bf16 = self._obs_bf16_store[:T], self._priv_bf16_store[:T]
        return True

    # ------------------------------------------------------------------ left-right symmetry augmentation
    MIRRORED = ("actions", "mu", "sigma", "values", "returns", "advantages", "actions_log_prob")

    def enable_mirror(self, spec):
        """Native extension (PPO.symmetry): room for the left-right mirrored transition of every stored row, in every column the update
        gathers -- observations and privileged observations (fp32 and, with enable_shadow, the bf16 shadows), actions, mu, sigma, values,
        returns, advantages, actions_log_prob.  spec: a humanoid.utils.symmetry.MirrorSpec whose table widths are this storage's.

        Addressing: each of those columns becomes ONE allocation of 2 T + 1 slots of N rows -- slots 0 .. T - 1 the rollout (what the
        attributes of the same names keep showing, shapes unchanged), slot T the bootstrap observation (unused in the other columns),
        slots T + 1 .. 2 T the mirrored rollout.  The update still gets one base pointer per column and one index slice: row r < T N is
        row r, mirrored row T N + r is row (T + 1) N + r (mirror_index).  Call it before anything binds the slots' addresses."""
        if self._priv_all is None:
            raise ValueError("enable_mirror needs privileged observations (the update's critic rows)")
        widths = (self.obs_shape[0], self.privileged_obs_shape[0], self.actions_shape[0])
        if (len(spec.obs_src), len(spec.priv_src), len(spec.act_src)) != widths:
            raise ValueError("MirrorSpec tables are %d / %d / %d wide, the storage's rows %d / %d / %d"
                             % ((len(spec.obs_src), len(spec.priv_src), len(spec.act_src)) + widths))
        T, N = self.num_transitions_per_env, self.num_envs

        def grow(t, keep):      # (keep leading slots of t) -> a zero-filled (2 T + 1)-slot allocation holding them
            g = torch.zeros(2 * T + 1, *t.shape[1:], dtype=t.dtype, device=self.device)
            g[:keep].copy_(t[:keep])
            return g
        self._obs_store, self._priv_store = grow(self._obs_all, T + 1), grow(self._priv_all, T + 1)
        self._obs_all, self._priv_all = self._obs_store[:T + 1], self._priv_store[:T + 1]
        self.observations, self.privileged_observations = self._obs_store[:T], self._priv_store[:T]
        self._col_store = {}
        for name in self.MIRRORED:
            self._col_store[name] = grow(getattr(self, name), T)
            setattr(self, name, self._col_store[name][:T])
        dev = lambda v, dt: torch.tensor(v, dtype=dt, device=self.device)
        self._mirror = dict(spec=spec, obs=(dev(spec.obs_src, torch.int32), dev(spec.obs_sign, torch.float32)),
                            priv=(dev(spec.priv_src, torch.int32), dev(spec.priv_sign, torch.float32)),
                            act=(dev(spec.act_src, torch.int32), dev(spec.act_sign, torch.float32)),
                            sigma=(dev(spec.act_src, torch.int32), torch.ones(len(spec.act_src), dtype=torch.float32, device=self.device)),
                            hi=torch.empty(0, dtype=torch.bool, device=self.device))
        if self._obs_bf16 is not None:      # shadows allocated before: the same layout for them
            self.enable_shadow(self._obs_bf16.shape[2], self._priv_bf16.shape[2])
            self.shadow_valid = [False] * T
        return True

    @property
    def mirrored(self):
        return self._mirror is not None

    def mirror(self, observations_only=False):
        """observations_only (the mirror loss without augmentation, PPO.symmetry_augmentation = False): only the observation rows and
        their bf16 shadow -- the one column the update then reads behind the bootstrap slot (the actor's forward over the partner rows).
        Fill the mirrored half from the current rollout (after compute_returns, and after the deferred critic wrote values and the
        privileged shadow): hgym_mirror_rows per tensor, device copies for the four scalar columns, all on the current stream with
        fixed arguments (capturable).  The T N original rows and slot T are only read.  The bf16 shadows are mirrored from the shadows
        (a sign-bit flip commutes with the rounding), and only when every slot of them is valid -- otherwise the update does not read them."""
        import hgym
        m, T = self._mirror, self.num_transitions_per_env
        fl = lambda t: t.flatten(0, 1)
        hgym.mirror_rows(fl(self._obs_store[:T]), fl(self._obs_store[T + 1:]), *m["obs"])
        if observations_only:
            if self.shadows() is not None:
                hgym.mirror_rows(fl(self._obs_bf16_store[:T]), fl(self._obs_bf16_store[T + 1:]), *m["obs"], zero_to=self._obs_bf16_store.shape[2])
            return
        hgym.mirror_rows(fl(self._priv_store[:T]), fl(self._priv_store[T + 1:]), *m["priv"])
        for name, table in (("actions", "act"), ("mu", "act"), ("sigma", "sigma")):
            c = self._col_store[name]
            hgym.mirror_rows(fl(c[:T]), fl(c[T + 1:]), *m[table])
        if self.shadows() is not None:
            for store, table in ((self._obs_bf16_store, "obs"), (self._priv_bf16_store, "priv")):
                hgym.mirror_rows(fl(store[:T]), fl(store[T + 1:]), *m[table], zero_to=store.shape[2])
        for name in ("values", "returns", "advantages", "actions_log_prob"):
            c = self._col_store[name]
            c[T + 1:].copy_(c[:T])

    def mirror_index(self, perm):
        """Row numbers of [0, 2 T N) -- T N + r is the mirror of row r -- to rows of the (2 T + 1)-slot columns, in place: the upper half
        moves past slot T.  Two launches, no allocation after the first call."""
        T, N, m = self.num_transitions_per_env, self.num_envs, self._mirror
        with torch.inference_mode():
            if m["hi"].shape != perm.shape:
                m["hi"] = torch.empty(perm.shape, dtype=torch.bool, device=perm.device)
            torch.ge(perm, T * N, out=m["hi"])
            perm.add_(m["hi"], alpha=N)
        return perm

    def batch_columns(self):
        """(obs, priv, actions, values, advantages, returns, actions_log_prob, mu, sigma) flattened as hgym.make_batch takes them: T N rows,
        or all (2 T + 1) N rows of the enlarged columns with enable_mirror."""
        fl = lambda t: t.flatten(0, 1)
        if self._mirror is None:
            obs = fl(self.observations)
            priv = fl(self.privileged_observations) if self.privileged_observations is not None else obs
            return (obs, priv, fl(self.actions), self.values.view(-1), self.advantages.view(-1), self.returns.view(-1),
                    self.actions_log_prob.view(-1), fl(self.mu), fl(self.sigma))
        c = self._col_store
        return (fl(self._obs_store), fl(self._priv_store), fl(c["actions"]), c["values"].view(-1), c["advantages"].view(-1), c["returns"].view(-1),
                c["actions_log_prob"].view(-1), fl(c["mu"]), fl(c["sigma"]))

    def enable_deferred_values(self):
        """Native extension: columns for a rollout whose critic runs ONCE after collection (PPO.deferred_values): time_outs (T, N, 1)
        uint8 = the stale-by-design extras["time_outs"] the per-step bootstrap would have used (ppo.py:107-108), last_values (N, 1)."""
        if self.time_outs is None:
            T, N = self.num_transitions_per_env, self.num_envs
            self.time_outs = torch.zeros(T, N, 1, dtype=torch.uint8, device=self.device)
            self.last_values = torch.zeros(N, 1, dtype=torch.float32, device=self.device)

    def shadow_slot(self, s):
        """(obs_bf16[s], priv_bf16[s]) for the policy launch that reads slot s, which thereby becomes valid; None without shadows."""
        if self._obs_bf16 is None or s >= self.num_transitions_per_env:
            return None
        self.shadow_valid[s] = True
        return self._obs_bf16[s], self._priv_bf16[s]

    def shadows(self, mirrored=False):
        """The flattened (T*N, ld) shadows when every slot of the current rollout was written by its policy launch, else None.
        mirrored (enable_mirror): all (2 T + 1) N rows, laid out like batch_columns()."""
        if self._obs_bf16 is None or not all(self.shadow_valid):
            return None
        if mirrored and self._mirror is not None:
            return self._obs_bf16_store.flatten(0, 1), self._priv_bf16_store.flatten(0, 1)
        return self._obs_bf16.flatten(0, 1), self._priv_bf16.flatten(0, 1)

    # ------------------------------------------------------------------
    def _same(self, a, b):
        return a.data_ptr() == b.data_ptr() and a.shape == b.shape

    def add_transitions(self, transition):
        if self.step >= self.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        s = self.step
        # (name, destination, source, does the slot's bf16 shadow describe this column?)
        pairs = [("observations", self.observations[s], transition.observations, True), ("actions", self.actions[s], transition.actions, False),
                 ("rewards", self.rewards[s], transition.rewards.view(-1, 1), False), ("dones", self.dones[s], transition.dones.view(-1, 1), False),
                 ("values", self.values[s], transition.values, False),
                 ("actions_log_prob", self.actions_log_prob[s], transition.actions_log_prob.view(-1, 1), False),
                 ("mu", self.mu[s], transition.action_mean, False), ("sigma", self.sigma[s], transition.action_sigma, False)]
        if self.privileged_observations is not None:
            pairs.append(("privileged_observations", self.privileged_observations[s], transition.critic_observations, True))
        for name, dst, src, shadowed in pairs:
            if not self._same(dst, src):          # producers that already wrote the slot are not copied again
                dst.copy_(src)
                if shadowed:                      # observations copied in from elsewhere: the slot's bf16 shadow does not describe them
                    self.shadow_valid[s] = False
        self.step += 1

    def check_shadows(self, rows=64):
        """Debug aid (HGYM_CHECK_SHADOW=1: PPO.update calls it before gathering from the shadows): a few rows of every slot of the
        bf16 shadows against bfloat16(fp32 rows) -- catches a caller that wrote `observations[s]` directly behind the policy launch,
        which the validity flags cannot see."""
        sh = self.shadows()
        if sh is None:
            return
        T, N = self.num_transitions_per_env, self.num_envs
        idx = torch.randint(0, T * N, (rows,), device=self.device)
        for name, full, bf in (("observations", self.observations, sh[0]), ("privileged_observations", self.privileged_observations, sh[1])):
            want = full.flatten(0, 1)[idx].to(torch.bfloat16)
            got = bf[idx][:, :want.shape[1]]
            if not torch.equal(want, got):
                raise AssertionError("bf16 shadow of %s is stale: a storage slot was written behind the policy launch that shadowed it" % name)

    def clear(self):
        self.rotate()
        self.cleared()

    def rotate(self):       # clear()'s device part: the bootstrap observation (slot T) becomes slot 0 of the next rollout
        self._obs_all[0].copy_(self._obs_all[self.num_transitions_per_env])
        if self._priv_all is not None:
            self._priv_all[0].copy_(self._priv_all[self.num_transitions_per_env])

    def cleared(self):      # clear()'s host part (PPO._update_done: also behind a replayed update, whose graph holds the copies)
        self.step = 0
        self.shadow_valid = [False] * self.num_transitions_per_env

    def compute_returns(self, last_values, gamma, lam, stats_hook=None, time_outs=None, normalize=True):
        """rollout_storage.py:122-136.  time_outs (native extension, deferred values): `rewards` holds RAW rewards; the time-out
        bootstrap r += gamma * V * time_outs is applied (and written back) as the scan loads them (hgym_gae_bootstrap).
        normalize=False (native extension, PPO.advantage_normalization "minibatch" / "none"): rollout_storage.py:136 is left out --
        neither stats_hook nor hgym_adv_normalize runs, `advantages` stays returns - values as the scan wrote it."""
        from hgym import _lib as L
        T, N = self.num_transitions_per_env, self.num_envs
        if not self.rewards.is_cuda:
            raise RuntimeError("RolloutStorage.compute_returns runs on the HIP path only (storage is on %s)" % self.device)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        lv = last_values.reshape(N).contiguous()
        if time_outs is not None:
            L.check(L.lib.hgym_gae_bootstrap(T, N, L.fptr(self.rewards), L.fptr(self.values), L.u8ptr(self.dones), L.u8ptr(time_outs), L.fptr(lv),
                                             gamma, lam, L.fptr(self.returns), L.fptr(self.advantages), L.f64ptr(self._stats), s),
                    "hgym_gae_bootstrap")
        else:
            L.check(L.lib.hgym_gae(T, N, L.fptr(self.rewards), L.fptr(self.values), L.u8ptr(self.dones), L.fptr(lv), gamma, lam,
                                   L.fptr(self.returns), L.fptr(self.advantages), L.f64ptr(self._stats), s), "hgym_gae")
        if not normalize:
            return
        if stats_hook is not None:
            stats_hook(self._stats[:3])           # multi-GPU: all-reduce (sum, sumsq, count) for a global normalisation
        L.check(L.lib.hgym_adv_normalize(T * N, L.fptr(self.advantages), L.f64ptr(self._stats), s), "hgym_adv_normalize")

    def get_statistics(self):
        done = self.dones.clone()
        done[-1] = 1
        flat = done.permute(1, 0, 2).reshape(-1, 1)
        idx = torch.cat((flat.new_tensor([-1], dtype=torch.int64), flat.nonzero(as_tuple=False)[:, 0]))
        return (idx[1:] - idx[:-1]).float().mean(), self.rewards.mean()

    def permutation(self, n, seed, draw):
        """The minibatch permutation (reference :149, torch.randperm) as one hgym_randperm launch: a bijection of [0, n) keyed
        by (seed, draw), written into a buffer this object keeps.  draw: an int, or a one-element int64 DEVICE tensor holding it
        (hgym_randperm_dev: the launch's arguments are then the same in every iteration -- what a captured update replays)."""
        from hgym import _lib as L
        if getattr(self, "_perm", None) is None or self._perm.numel() != n:
            self._perm = torch.empty(n, dtype=torch.int64, device=self.device)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if torch.is_tensor(draw):
            assert draw.dtype == torch.int64 and draw.is_cuda and draw.numel() == 1
            L.check(L.lib.hgym_randperm_dev(n, int(seed) & 0xFFFFFFFFFFFFFFFF, L.i64ptr(draw), L.i64ptr(self._perm), s), "hgym_randperm_dev")
        else:
            L.check(L.lib.hgym_randperm(n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw), L.i64ptr(self._perm), s), "hgym_randperm")
        return self._perm

    def mini_batch_generator(self, num_mini_batches, num_epochs=8):
        """API-compatible generator (gathers with torch); the native PPO.update does not use it -- it hands the
        index slices to hgym_ppo_grad, which fuses the gather into the operand packing."""
        batch = self.num_envs * self.num_transitions_per_env
        mb = batch // num_mini_batches
        indices = torch.randperm(num_mini_batches * mb, requires_grad=False, device=self.device)
        fl = lambda t: t.flatten(0, 1)
        obs = fl(self.observations)
        cobs = fl(self.privileged_observations) if self.privileged_observations is not None else obs
        cols = [fl(self.actions), fl(self.values), fl(self.advantages), fl(self.returns), fl(self.actions_log_prob), fl(self.mu),
                fl(self.sigma)]
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                idx = indices[i * mb:(i + 1) * mb]
                a, v, adv, ret, lp, mu, sg = (c[idx] for c in cols)
                yield obs[idx], cobs[idx], a, v, adv, ret, lp, mu, sg, (None, None), None
