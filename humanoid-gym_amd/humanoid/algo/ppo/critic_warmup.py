"""PPO.critic_warmup_updates: the first n updates of a run move the value function alone.

A checkpoint without a usable critic -- a plain distillation run, an older policy, a changed reward -- starts PPO with advantages from a
random value function.  For n updates every minibatch step is hgym_vf_grad (keep_others = 0) followed by hgym_ppo_apply with the adaptive
learning-rate rule off: the actor's gradient is +0.0, and zero gradient on zero Adam moments moves nothing, so the actor, sigma and the
learning rate keep their bits.  The count of updates done is host state (a checkpoint carries it as STATE_KEY); while updates remain the
update's graph key says so, and the captured update is re-captured once at the switch.
"""
import torch

STATE_KEY = "critic_warmup_state_dict"      # what a checkpoint of a run with PPO.critic_warmup_updates > 0 carries: done, updates


def parse_config(n):
    """PPO.critic_warmup_updates -> the number of critic-only updates (0: off).  ValueError for anything but an integer >= 0."""
    if n is None:
        return 0
    if isinstance(n, bool) or int(n) != n or int(n) < 0:
        raise ValueError("PPO.critic_warmup_updates=%r: must be an integer >= 0" % (n,))
    return int(n)


def check_setup(world=1):
    """What init_storage refuses with the option on (ValueError): more than one rank (hgym_vf_grad is a one-rank call)."""
    if int(world) > 1:
        raise ValueError("PPO.critic_warmup_updates runs on one rank (world size %d)" % int(world))


def check_moments(remaining, named_moments):
    """Updates remain and an optimiser state with non-zero Adam moments of std / log_std or the actor arrives: ValueError -- a zero
    gradient on non-zero moments would move the actor.  named_moments: (name, exp_avg, exp_avg_sq) of every parameter tensor."""
    if remaining <= 0:
        return
    for name, m, v in named_moments:
        if name.startswith("critic."):
            continue
        if bool((torch.as_tensor(m) != 0).any()) or bool((torch.as_tensor(v) != 0).any()):
            raise ValueError("PPO.critic_warmup_updates: %d critic-only updates remain, but the optimiser state has non-zero Adam moments "
                             "for `%s`; a zero gradient on them would move the actor (load the model without its optimiser state)" % (remaining, name))


def check_state_dict(sd, name, on):
    """A checkpoint with STATE_KEY for a run without the option, or the reverse: refused by key name."""
    if sd is not None and not on:
        raise RuntimeError("%s carries `%s`: it was trained with PPO.critic_warmup_updates, this run was built without it" % (name, STATE_KEY))
    if sd is None and on:
        raise RuntimeError("%s has no `%s`: it was trained without PPO.critic_warmup_updates, this run was built with it" % (name, STATE_KEY))


class CriticWarmup:
    """The option as PPO holds it (PPO._warmup; None: off).  `done`: the number of updates completed (host state).  `active`: critic-only
    updates remain -- once none does, update() is the plain one and the graph key says so."""

    def __init__(self, updates, ppo_cfg, clip_param, value_loss_coef, clipped, device):
        import hgym
        self._hgym = hgym
        self.updates, self.done = int(updates), 0
        self.vf_cfg = hgym.make_vf_config(clip_param, value_loss_coef, clipped_value_loss=clipped, keep_others=False)
        # the step is hgym_ppo_apply's with the run's own clip and Adam, the learning-rate rule off (the actor does not move: the KL is 0
        # and the rule would multiply the learning rate at every step) and the norm from its own pass (hgym_vf_grad takes no prologue)
        self.apply_cfg = type(ppo_cfg).from_buffer_copy(ppo_cfg)
        self.apply_cfg.adaptive_lr, self.apply_cfg.grad_norm_ready = 0, 0
        self.block = torch.zeros(3, dtype=torch.float64, device=device)      # [0] the sum of the minibatches' value losses, [1] their number, [2] updates remaining behind the last critic-only one
        self.sums = self.block[0:2]
        self._retired = False
        self.last = None

    @property
    def remaining(self):
        return max(self.updates - self.done, 0)

    @property
    def active(self):
        return self.remaining > 0

    def begin_update(self):
        """The start of a critic-only update: the two sums zeroed, the count the log reads moved on.  Eager calls re-seat the device count
        from the host's first (what a resume set); under capture nothing is re-seated -- replays continue the device count."""
        with torch.inference_mode():
            if not torch.cuda.is_current_stream_capturing():
                self.block[2:3].fill_(float(self.remaining))
            self.block[0:2] = 0.0      # (a slice: a fill kernel)
            self.block[2:3].sub_(1.0)

    def update_done(self):
        self.done += 1

    def retire_if_done(self):
        """Once, outside any capture, when no update remains: the log's three numbers to 0, so that the plain rest of the run reads its
        value loss from opt_state again without any launch of the option in the update."""
        if not self.active and not self._retired and not torch.cuda.is_current_stream_capturing():
            with torch.inference_mode():
                self.block[0:3] = 0.0
            self._retired = True

    def graph_key(self):
        return dict(critic_warmup=self.active)

    def log_parts(self):
        return [("critic_warmup", self.block)]

    def read_log(self, parts):
        """`last` = {value_loss, remaining} from the parts of a host copy of PPO.log_block(); value_loss None behind a plain update."""
        s, n, rem = (float(x) for x in parts["critic_warmup"])
        self.last = dict(value_loss=s / n if n > 0 else None, remaining=int(rem) + 1 if n > 0 else 0, trained=n > 0)      # remaining: this update included
        return self.last

    def log_scalars(self):
        if self.last is None or not self.last["trained"]:
            return []
        return [("Policy/critic_warmup_remaining", float(self.last["remaining"]))]

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        return dict(done=int(self.done), updates=int(self.updates))

    def load_state_dict(self, sd):
        self.done = int(sd["done"])
        self._retired = False
        self.retire_if_done()
