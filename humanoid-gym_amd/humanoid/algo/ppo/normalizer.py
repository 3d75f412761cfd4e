"""What `ActorCritic.obs_normalizer` / `critic_obs_normalizer` expose (rsl_rl's EmpiricalNormalization, seen from the host).

The statistics live on the device, in the block a hgym.NetBuffers owns (HgymNet.norm), and the kernels never call this module: the
normaliser is folded into the first layer of every net.  `mean`, `var`, `std`, `count` read that state; `forward`
is the plain torch expression for host-side users (plots, a policy evaluated outside the kernels).  Before the ActorCritic is bound to a
net the module holds the initial state itself: mean 0, var 1, count 0."""
import math

import torch
import torch.nn as nn


class EmpiricalNormalization(nn.Module):
    def __init__(self, num_columns, eps=1e-2, until=None, which=0):
        """which: 0 -- the actor's statistics (num_obs columns, shared by the denoiser head), 1 -- the critic's (num_priv)."""
        super().__init__()
        self.num_columns, self.eps, self.until, self.which = int(num_columns), float(eps), until, int(which)
        self._net = None

    def bind(self, net):
        self._net = net
        return self

    def _part(self, name):
        if self._net is not None:
            return self._net.norm_view(name, self.which)
        return torch.zeros(self.num_columns, dtype=torch.float64) if name == "mean" else torch.ones(self.num_columns, dtype=torch.float64)

    @property
    def mean(self):
        return self._part("mean").clone()

    @property
    def var(self):
        return self._part("var").clone()

    @property
    def std(self):
        return torch.sqrt(self._part("var"))

    @property
    def count(self):
        return 0 if self._net is None else int(self._net.norm_view("header")[2 + self.which])

    def forward(self, x):
        """(x - mean) / (std + eps) with the state as it is now, in x's dtype and on x's device."""
        m = self._part("mean").to(device=x.device, dtype=x.dtype)
        s = torch.sqrt(self._part("var")).to(device=x.device, dtype=x.dtype)
        return (x - m) / (s + self.eps)

    def norm_state_dict(self):
        """mean, var (fp64, cpu), count, eps, until: the checkpoint entry of this normaliser."""
        return dict(mean=self._part("mean").detach().cpu().clone(), var=self._part("var").detach().cpu().clone(), count=float(self.count),
                    eps=self.eps, until=self.until)


class ValueNormalizer:
    """PPO.value_normalization as PPO holds it (`PPO.value_normalizer`; None: off): the running statistics of the raw
    returns -- `block`, three doubles (count, mean, var) on the device --, the launches that use them, and the host's view of them.

    The launches (on_device() allocates what they name): whoever fills the storage's `values` follows with denormalize(), compute_returns()
    runs GAE on raw values, and normalize_targets() behind it puts `returns` and `values` into the critic's units for the update.

    The host's view: every property reads a host copy of the block (a synchronising read-back), `forward` / `inverse` are the plain torch
    expressions for host-side users -- a critic evaluated outside the kernels returns normalised values (ActorCritic.evaluate), inverse()
    turns them into raw ones.  Not for the training loop: each property, and each forward / inverse call, waits for the device; a caller
    that wants several numbers takes them from ONE read, stats().  `block` is the device tensor itself (what a checkpoint snapshot copies
    stream-side, without a wait)."""

    def __init__(self, block, eps, scratch=None, last_values=None):
        """scratch, last_values: hgym_value_norm_merge's scratch and the (N, 1) buffer of the denormalised bootstrap value; the host's view
        needs neither."""
        self.block, self.eps, self.scratch, self.last_values, self.last = block, float(eps), scratch, last_values, None

    @classmethod
    def on_device(cls, eps, num_values, num_envs, device):
        """The statistics at (0, 0, 1) and the scratch for merging num_values (T N) returns at a time, all allocated once."""
        from hgym import _lib as L
        return cls(L.value_norm_block(device), eps, L.value_norm_scratch(num_values, device),
                   torch.zeros(num_envs, 1, dtype=torch.float32, device=device))

    def denormalize(self, v, out=None):
        """out (default: v itself) = v * scale_f + mean_f under the statistics as they are (hgym_value_denormalize: one launch, fixed
        arguments -- capturable): the critic's outputs -> raw values.  v: any contiguous fp32 column."""
        import hgym
        return hgym.value_denormalize(v.view(-1), self.block, self.eps, None if out is None else out.view(-1))

    def normalize_targets(self, returns, values):
        """Behind compute_returns(): merge the raw returns into the statistics FIRST (hgym_value_norm_merge), then returns <- normalise(returns)
        and values <- normalise(values) in place under the NEW statistics (hgym_value_normalize twice): three launches, fixed arguments."""
        import hgym
        hgym.value_norm_merge(returns.view(-1), self.block, self.scratch)
        hgym.value_normalize(returns.view(-1), self.block, self.eps)
        hgym.value_normalize(values.view(-1), self.block, self.eps)

    def graph_key(self):
        """PPO.update_graph_key's entry (and the tail of rollout_graph_key): eps and the two buffers the launches name."""
        return dict(value_norm=(self.eps, self.block.data_ptr(), self.scratch.data_ptr()))

    def log_parts(self):
        return [("value_norm", self.block)]

    def read_log(self, parts):
        """`last` = {count, mean, var, std} from the parts of a host copy of PPO.log_block()."""
        count, mean, var = (float(x) for x in parts["value_norm"])
        self.last = dict(count=count, mean=mean, var=var, std=math.sqrt(max(var, 0.0)))
        return self.last

    def log_scalars(self):
        return [] if self.last is None else [("Policy/value_norm_mean", self.last["mean"]), ("Policy/value_norm_std", self.last["std"])]

    def _host(self):
        return self.block.detach().cpu()

    def stats(self):
        """{count, mean, var, std} as python numbers from one read-back."""
        count, mean, var = (float(x) for x in self._host())
        return dict(count=int(count), mean=mean, var=var, std=math.sqrt(max(var, 0.0)))

    @property
    def count(self):
        return int(self._host()[0])

    @property
    def mean(self):
        return self._host()[1].clone()

    @property
    def var(self):
        return self._host()[2].clone()

    @property
    def std(self):
        return torch.sqrt(self._host()[2])

    def _floats(self, x):
        b = self._host()
        return b[1].to(device=x.device, dtype=x.dtype), torch.sqrt(b[2]).to(device=x.device, dtype=x.dtype) + self.eps

    def forward(self, x):
        """(x - mean) / (std + eps): raw returns or values -> the critic's units, in x's dtype and on x's device."""
        m, s = self._floats(x)
        return (x - m) / s

    __call__ = forward

    def inverse(self, y):
        """y * (std + eps) + mean: the critic's outputs -> raw values."""
        m, s = self._floats(y)
        return y * s + m

    def state_dict(self):
        """count, mean, var, eps as python floats: the checkpoint entry (value_norm_state_dict)."""
        b = self._host()
        return dict(count=float(b[0]), mean=float(b[1]), var=float(b[2]), eps=self.eps)

    def load_state_dict(self, sd):
        """The three doubles back onto the device (python floats are doubles: the same bits)."""
        self.block.copy_(torch.tensor([float(sd["count"]), float(sd["mean"]), float(sd["var"])], dtype=torch.float64))
