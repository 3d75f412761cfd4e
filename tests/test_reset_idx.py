"""CPU side of LeggedRobot.reset_idx(env_ids) for a subset of envs: the host id normalisation, the recorded reference trace against the
oracle (so the fixture and the oracle are known to agree before any GPU time), and the fixture generator's determinism."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reset_idx_golden as RG
from humanoid.envs.base.legged_robot import host_env_ids
from reset_idx_common import reset_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reset_mask_wraps_dedupes_and_skips():
    N = 10
    m = reset_mask([3, -1, 3, 0, -10, 10, -11], N)
    want = torch.zeros(N, dtype=torch.bool)
    want[[3, 9, 0]] = True                   # -1 -> 9, -10 -> 0; 10 and -11 are out of range (the device counts them as rejected)
    assert torch.equal(m, want)
    ref = torch.zeros(N, dtype=torch.bool)
    ids = torch.tensor([7, -3, 7, 2])
    ref[ids] = True                          # torch indexing: the same envs
    assert torch.equal(reset_mask(ids, N), ref) and torch.equal(reset_mask(ids.numpy(), N), ref)


def test_host_ids_forms_and_range_errors():
    N = 8
    for form in ([1, -8, 7], np.array([1, -8, 7]), torch.tensor([1, -8, 7], dtype=torch.int32), (1, -8, 7)):
        t = host_env_ids(form, N)
        assert t.dtype == torch.int64 and t.is_contiguous() and t.tolist() == [1, -8, 7]
    for bad in ([8], [-9], np.array([0, 100]), torch.tensor([3, -20])):
        with pytest.raises(IndexError):
            host_env_ids(bad, N)
    for bad in ([0.5], torch.tensor([True, False]), np.array([1.0, 2.0])):
        with pytest.raises(IndexError):
            host_env_ids(bad, N)


FIXTURES = ["reset_idx_trace.npz", "reset_idx_trace_generic.npz"]      # XBot-L defaults | trimesh map, terrain + command curricula


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_reset_idx(golden_dir, name):
    RG.run_reset_idx_golden(None, os.path.join(golden_dir, name))


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference tree is not on this machine")
def test_fixture_generator_is_deterministic(tmp_path, golden_dir):
    gen = os.path.join(golden_dir, "gen_reset_idx_fixture.py")
    subprocess.run([sys.executable, gen, str(tmp_path)], check=True, cwd=ROOT, capture_output=True, timeout=600)
    for name in FIXTURES:
        with open(os.path.join(tmp_path, name), "rb") as a, open(os.path.join(golden_dir, name), "rb") as b:
            assert a.read() == b.read(), name
