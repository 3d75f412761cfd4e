"""The mirror loss as PPO holds it (PPO.mirror_loss_coef > 0: PPO._mirror_loss; None: off): the coefficient, the
pre-pass's output, the two sums behind the logged loss.  The mirrored observations it reads are columns of the storage
(RolloutStorage.enable_mirror / mirror)."""
import torch

from .log_block import mean_of_sums
from .rollout_storage import mirror_pair_rows


class MirrorLoss:
    def __init__(self, coef, mb, num_actions, device):
        """target: one minibatch (mb rows) of raw partner means; sums: [sum of the MSE, minibatches].  Allocated once."""
        self.coef, self.last = float(coef), None
        self.target = torch.zeros(max(mb, 1) * num_actions, dtype=torch.float32, device=device)
        self.sums = torch.zeros(2, dtype=torch.float64, device=device)

    def begin_update(self, perm, storage):
        """-> every drawn row's partner, original or mirrored (without augmentation only rows < T N are drawn), for every epoch."""
        pair = mirror_pair_rows(perm, storage.num_transitions_per_env, storage.num_envs)
        self.sums[0:2] = 0.0      # (a slice: a fill kernel)
        return pair

    def minibatch(self, pair, storage):
        """hgym.make_batch's keywords for the minibatch whose rows' partners are `pair` (its slice of begin_update's)."""
        return dict(pair_idx=pair, mirror=storage._mirror["act"] + (self.target, self.sums))

    def graph_key(self):
        """PPO.update_graph_key's entries: the coefficient (also part of ppo_cfg's bytes) and the scratch the launches name."""
        return dict(mirror_coef=self.coef, mirror_scratch=(self.target.data_ptr(), self.sums.data_ptr()))

    def log_parts(self):
        return [("mirror", self.sums)]

    def read_log(self, parts):
        """`last` = the mean mirror MSE per minibatch from the parts of a host copy of PPO.log_block()."""
        self.last = mean_of_sums(parts["mirror"])
        return self.last

    def log_scalars(self):
        return [] if self.last is None else [("Loss/mirror", self.last)]
