"""The log block of an update: the device tensors a log line reads, copied to the host as ONE tensor and taken apart again by name.

PPO.init_storage lists `opt` (opt_state) and, behind it, the log_parts() of every option that is on (PPO._log_parts); the order of the
list is the byte layout (checkpoints, tools and tests hold such blocks):  PPO  opt | mirror(2) | rnd_sums(2) | rnd_block(RND_HEADER) |
smooth(4) | value_norm(3);  Distillation  opt | bc(2).  Plain torch, no device needed."""
import torch


def mean_of_sums(part):
    """A part of two numbers [sum of a loss, number of steps it was taken on] -> the mean per step (at least 1 step); None -> None."""
    return None if part is None else float(part[0]) / max(float(part[1]), 1.0)


class LogBlock:
    def __init__(self, parts):
        """parts: [(name, 1-D tensor)] in layout order; distinct names, one dtype (torch.cat would promote)."""
        self.parts = list(parts)
        assert len({n for n, _ in self.parts}) == len(self.parts) and all(t.dim() == 1 and t.dtype == self.parts[0][1].dtype for _, t in self.parts)

    def numel(self):
        return sum(t.numel() for _, t in self.parts)

    def device(self):
        """The tensor to copy to the host: the one part itself when there is no other, else their concatenation (one launch)."""
        return self.parts[0][1] if len(self.parts) == 1 else torch.cat([t for _, t in self.parts])

    def split(self, block):
        """A copy of device(), on the host or not -> {name: view of its part}."""
        assert block.numel() == self.numel(), "a log block of %d numbers, %d listed" % (block.numel(), self.numel())
        sizes = [t.numel() for _, t in self.parts]
        return dict(zip((n for n, _ in self.parts), block.split(sizes)))
