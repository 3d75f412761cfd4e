"""What `ActorCritic.obs_normalizer` / `critic_obs_normalizer` expose (rsl_rl's EmpiricalNormalization, seen from the host).

The statistics live on the device, in the block a hgym.NetBuffers owns (HgymNet.norm), and the kernels never call this module: the
normaliser is folded into the first layer of every net.  `mean`, `var`, `std`, `count` read that state; `forward`
is the plain torch expression for host-side users (plots, a policy evaluated outside the kernels).  Before the ActorCritic is bound to a
net the module holds the initial state itself: mean 0, var 1, count 0."""
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
