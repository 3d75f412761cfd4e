"""StudentTeacher: the policy of rsl_rl's Distillation -- a student MLP that is trained to reproduce a frozen teacher MLP.

A subclass of ActorCritic whose `actor` IS the student, so everything that serves an ActorCritic serves a distilled policy unchanged:
export_policy_as_jit, act_inference, OnPolicyRunner.evaluate, play.py and the fused rollout.  One more module, `teacher`, holds the
network that is cloned; it is never trained.  The critic is kept and left untrained: a distillation checkpoint minus its `teacher.*` keys
is a valid PPO checkpoint (student_state_dict).

State-dict keys: ActorCritic's (`std` | `log_std`, `actor.*`, `critic.*`), followed by `teacher.<i>.weight/bias`.  rsl_rl names the
student `student.*`; here it keeps the name every other tool of this repository reads.

On the device the teacher lives in a second hgym.NetBuffers of its own, in the actor slot, beside a placeholder critic of widths the
fused bf16 kernels accept -- the library picks the fused path by looking at both trunks.
"""
import torch
import torch.nn as nn

from .actor_critic import ActorCritic, _mlp

PLACEHOLDER_CRITIC_DIMS = [256, 128, 128]      # the smallest trunk the fused bf16 kernels take; never evaluated, never trained
TEACHER_MAX_BATCH = 16384      # rows per launch of the teacher's pass by default: one 64-row tile per CU of a 256-CU device


def forward_in_pieces(net, x, y, which=0):
    """Net `which` of a NetBuffers over all M rows of x ((M, in) fp32 contiguous) into y ((M, out) fp32 contiguous), in pieces of at most
    max_batch rows (whole 64-row tiles when max_batch allows) -- one hgym_mlp_forward per piece, nothing allocated."""
    import ctypes as C
    from hgym import _lib as L
    assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.float32 and x.shape[0] == y.shape[0]
    M, mb = int(x.shape[0]), int(net.cfg.max_batch)
    piece = mb if mb < 64 else mb // 64 * 64
    for m0 in range(0, M, piece):
        m = min(piece, M - m0)
        a, b = x[m0:m0 + m], y[m0:m0 + m]
        L.check(L.lib.hgym_mlp_forward(C.byref(net.cfg), C.byref(net.struct), which, m, L.fptr(a), a.stride(0), L.fptr(b), net.stream()),
                "hgym_mlp_forward")
    return y


class StudentTeacher(ActorCritic):
    # rows per launch of the teacher's pass over the stored observations (teacher_pass); None: see bind()
    teacher_max_batch = None

    def __init__(self, num_actor_obs, num_critic_obs, num_actions, student_hidden_dims=[256, 128, 128],
                 teacher_hidden_dims=[512, 256, 128], critic_hidden_dims=[768, 256, 128], activation=nn.ELU(), init_noise_std=0.1,
                 noise_std_type="scalar", fused_activation=None, empirical_normalization=False, **kwargs):
        if empirical_normalization:
            raise ValueError("StudentTeacher(empirical_normalization=True) is not supported: a teacher trained with normalisation carries "
                             "statistics that its first layer would have to fold in")
        super().__init__(num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=student_hidden_dims,
                         critic_hidden_dims=critic_hidden_dims, init_noise_std=init_noise_std, activation=activation,
                         fused_activation=fused_activation, noise_std_type=noise_std_type, **kwargs)
        if self.denoiser_hidden_dims:
            raise ValueError("StudentTeacher: the auxiliary (denoiser) head is not trained during distillation and is not supported")
        self.student_hidden_dims, self.teacher_hidden_dims = list(student_hidden_dims), list(teacher_hidden_dims)
        self.teacher = _mlp([num_actor_obs] + self.teacher_hidden_dims + [num_actions], activation)
        for p in self.teacher.parameters():
            p.requires_grad_(False)
        print(f"Teacher MLP: {self.teacher}")
        self.loaded_teacher = False
        self._teacher_net = None

    # ------------------------------------------------------------------ binding to the HIP path
    def bind(self, net):
        """The student, the critic and sigma alias `net` (ActorCritic.bind); the teacher a NetBuffers of its own, built here with the
        same precision and activation.  It only ever runs forwards, in pieces of its max_batch: teacher_max_batch if set, else the
        student's max_batch capped at TEACHER_MAX_BATCH rows, which keeps its workspace -- proportional to max_batch -- small."""
        import hgym
        teacher = self._modules.pop("teacher")      # ActorCritic.bind walks named_parameters(): the teacher's are not in `net`
        try:
            super().bind(net)
        finally:
            self._modules["teacher"] = teacher
        mb = int(self.teacher_max_batch) if self.teacher_max_batch else min(int(net.cfg.max_batch), TEACHER_MAX_BATCH)
        cfg = hgym.make_net_config(self.num_actor_obs, self.num_critic_obs, self.num_actions, self.teacher_hidden_dims,
                                   PLACEHOLDER_CRITIC_DIMS, int(net.cfg.precision), mb, activation=self.activation,
                                   fused_activation=self.fused_activation, noise_std_type=self.noise_std_type)
        tnet = hgym.NetBuffers(cfg, net.device)
        tnet.params[:self.num_actions] = 1.0 if self.noise_std_type != "log" else 0.0      # a valid sigma; nothing reads it
        with torch.no_grad():
            for name, p in self.teacher.named_parameters():
                view = tnet.views["actor." + name]
                view.copy_(p.detach().to(view.device))
                p.data = view
        tnet.sync_shadow()
        self._teacher_net = tnet
        return self

    # ------------------------------------------------------------------ state dicts
    def student_state_dict(self):
        """The state dict without its `teacher.*` entries: loads strictly into ActorCritic(..., actor_hidden_dims=student_hidden_dims)."""
        return {k: v for k, v in self.state_dict().items() if not k.startswith("teacher.")}

    def load_state_dict(self, state_dict, strict=True):
        """Two cases.  A dict WITHOUT `teacher.*` keys is a teacher's PPO checkpoint (this repository's, the reference's or rsl_rl's):
        its `actor.*` tensors go into `teacher.*`, shapes checked by name; `std` and `critic.*` are ignored; returns False ("not a
        resume").  A dict WITH `teacher.*` keys is a distillation checkpoint: everything is loaded strictly; returns True."""
        if any(k.startswith("teacher.") for k in state_dict):
            super().load_state_dict(state_dict, strict=True)
            self._teacher_loaded()
            return True
        own = self.teacher.state_dict()
        theirs = {k[len("actor."):]: v for k, v in state_dict.items() if k.startswith("actor.")}
        missing, extra = sorted(set(own) - set(theirs)), sorted(set(theirs) - set(own))
        if missing or extra:
            raise RuntimeError("teacher checkpoint does not fit teacher_hidden_dims=%r: missing %s, unexpected %s"
                               % (self.teacher_hidden_dims, ["actor." + k for k in missing], ["actor." + k for k in extra]))
        for k, v in own.items():
            if tuple(theirs[k].shape) != tuple(v.shape):
                raise RuntimeError("teacher checkpoint: actor.%s has shape %s, teacher.%s needs %s (teacher_hidden_dims=%r)"
                                   % (k, tuple(theirs[k].shape), k, tuple(v.shape), self.teacher_hidden_dims))
        with torch.no_grad():
            for k, p in self.teacher.named_parameters():
                p.copy_(torch.as_tensor(theirs[k]).to(device=p.device, dtype=p.dtype))
        self._teacher_loaded()
        return False

    def _teacher_loaded(self):
        if self._teacher_net is not None:
            self._teacher_net.sync_shadow()
        self.loaded_teacher = True

    # ------------------------------------------------------------------ the teacher on the device
    def _need_teacher_net(self):
        if self._teacher_net is None:
            raise RuntimeError("StudentTeacher is not bound to the HIP network (Distillation binds it); the teacher has no CPU path here")
        return self._teacher_net

    def teacher_inference(self, observations):
        """The teacher's mean action for every row of `observations` (at most the teacher net's max_batch rows): hgym_mlp_forward(which=0)."""
        return self._need_teacher_net().forward(0, observations.contiguous())

    def teacher_pass(self, observations, out):
        """The teacher over all M rows of `observations` ((M, num_obs) fp32 contiguous) into `out` ((M, num_actions) fp32 contiguous), in
        pieces of at most max_batch rows (whole 64-row tiles when max_batch allows) -- one hgym_mlp_forward per piece, nothing allocated."""
        net = self._need_teacher_net()
        assert out.shape[0] == observations.shape[0] and out.shape[1] == self.num_actions
        return forward_in_pieces(net, observations, out)
