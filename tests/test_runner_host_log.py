"""CPU: the host side of OnPolicyRunner's logging book-keeping (_EpisodeLog, what a logging run keeps when the step finaliser's log sink
is off) against the reference's loop (on_policy_runner.py:144-154) on planted rewards and dones: cur_reward_sum / cur_episode_length
and the two deque(maxlen=100) buffers, episode by episode and in order."""
from collections import deque

import pytest
import torch

from humanoid.algo.ppo.on_policy_runner import _EpisodeLog


@pytest.mark.parametrize("N", [1, 37, 264, 1001])
def test_host_episode_log_keeps_the_reference_deques(N):
    g = torch.Generator().manual_seed(N)
    log = _EpisodeLog(True, _EpisodeLog.tensors(N, "cpu"))
    rewbuffer, lenbuffer = deque(maxlen=100), deque(maxlen=100)
    cur_reward_sum, cur_episode_length = torch.zeros(N), torch.zeros(N)
    ones, none = torch.ones(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
    first, last = none.clone(), none.clone()
    first[0], last[-1] = True, True
    pick = lambda k: torch.zeros(N, dtype=torch.bool).index_fill_(0, torch.randperm(N, generator=g)[:k], True)
    masks = [none, first, last, pick(60), pick(60), pick(100), pick(101), none, ones, torch.rand(N, generator=g) < 0.3, ones, pick(7)]
    for t, dones in enumerate(masks):
        rewards = torch.randn(N, generator=g)
        dones = dones.to(torch.uint8) if t % 2 else dones            # the env hands out either
        log.step(rewards, dones)
        cur_reward_sum += rewards
        cur_episode_length += 1
        new_ids = (dones > 0).nonzero(as_tuple=False)
        rewbuffer.extend(cur_reward_sum[new_ids][:, 0].cpu().numpy().tolist())
        lenbuffer.extend(cur_episode_length[new_ids][:, 0].cpu().numpy().tolist())
        cur_reward_sum[new_ids] = 0
        cur_episode_length[new_ids] = 0
        got_r, got_l = log.read()
        assert list(got_r) == list(rewbuffer) and list(got_l) == list(lenbuffer), t
        assert torch.equal(log.reward_sum, cur_reward_sum) and torch.equal(log.length, cur_episode_length), t
        assert int(log.meta[1]) == len(rewbuffer) <= 100
