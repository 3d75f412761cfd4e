"""CPU-only: the named log block (humanoid/algo/ppo/log_block.py) and what PPO builds on it, on CPU tensors and stand-in objects.

1. Layout: every on/off combination of PPO's three tails and Distillation's block -- device() is the hand-written concatenation
   opt | mirror(2) | rnd sums(2) | rnd block head(RND_HEADER) | smooth(4)  /  opt | bc(2), split() names exactly the parts that are on, and
   an option-free block IS opt_state.
2. The options' readers (read_log of MirrorLoss, Smoothness and RND; Distillation.behavior_loss_from) against the offset arithmetic they replace.
3. PPO.check_setup: every refusal with its message, the order in which they win, Distillation's refusals ahead of them -- no device."""
import itertools
import re
from types import SimpleNamespace

import pytest
import torch

from hgym import _lib as L
from humanoid.algo import PPO, Distillation, RandomNetworkDistillation as RND
from humanoid.algo.ppo.log_block import LogBlock
from humanoid.algo.ppo.mirror_loss import MirrorLoss
from humanoid.algo.ppo.smoothness import Smoothness

MB = 4
f64 = lambda *v: torch.tensor(v, dtype=torch.float64)


def _option(cls, **fields):
    """An option object made without __init__ (which allocates on a device): the fields its log side uses."""
    o = object.__new__(cls)
    o.__dict__.update(dict(last=None), **fields)
    return o


def _rnd(**fields):
    """The same for RND (an nn.Module): a stand-in that borrows its log methods."""
    r = SimpleNamespace(**fields)
    r.log_parts, r.log_from, r.read_log, r.log_scalars = (lambda: RND.log_parts(r)), (lambda tail: RND.log_from(r, tail)), \
        (lambda parts: RND.read_log(r, parts)), (lambda: RND.log_scalars(r))
    return r


def _alg(mirror=None, rnd=None, smooth=None, bc=None):
    """A stand-in for a PPO (or, with bc, a Distillation) behind init_storage: the fields _log_parts and the readers use.  mirror,
    smooth, bc: the part's tensor or None (off); rnd: (sums, block) or None."""
    opt = torch.arange(1.0, L.OPT_STATE + 1.0, dtype=torch.float64)
    a = SimpleNamespace(net=SimpleNamespace(opt_state=opt), _mirror_loss=None if mirror is None else _option(MirrorLoss, sums=mirror),
                        _rnd=None if rnd is None else _rnd(sums=rnd[0], block=rnd[1]),
                        _smooth=None if smooth is None else _option(Smoothness, sums=smooth, mb=MB), value_normalizer=None, _bc_sums=bc)
    a._options = tuple(o for o in (a._mirror_loss, a._rnd, a._smooth, a.value_normalizer) if o is not None)
    a._log = LogBlock((PPO if bc is None else Distillation)._log_parts(a))
    return a


def _read(a, option, block):
    """Option `option` of stand-in `a` reads its numbers from a host copy of the log block; None when it is off."""
    o = getattr(a, option)
    return None if o is None else o.read_log(a._log.split(block))


mirror_loss_from = lambda a, block: _read(a, "_mirror_loss", block)
smoothness_from = lambda a, block: _read(a, "_smooth", block)
rnd_log_from = lambda a, block: _read(a, "_rnd", block)


def _tails():
    """Distinct values per part; the RND block is longer than its head, as the real one is."""
    return dict(mirror=f64(21.0, 22.0), rnd=(f64(31.0, 32.0), torch.arange(100.0, 100.0 + L.RND_HEADER + 9, dtype=torch.float64)),
                smooth=f64(41.0, 42.0, 43.0, 44.0))


@pytest.mark.parametrize("on", list(itertools.product((False, True), repeat=3)), ids=lambda on: "".join("MRS"[i] if b else "-" for i, b in enumerate(on)))
def test_ppo_layout(on):
    t = _tails()
    a = _alg(**{k: (t[k] if b else None) for k, b in zip(("mirror", "rnd", "smooth"), on)})
    opt = a.net.opt_state
    want, names = [opt], ["opt"]
    if on[0]:
        want, names = want + [t["mirror"]], names + ["mirror"]
    if on[1]:
        want, names = want + [t["rnd"][0], t["rnd"][1][:L.RND_HEADER]], names + ["rnd_sums", "rnd_block"]
    if on[2]:
        want, names = want + [t["smooth"]], names + ["smooth"]
    block = a._log.device()
    assert torch.equal(block, torch.cat(want)) and a._log.numel() == block.numel()
    assert block.numel() == L.OPT_STATE + 2 * on[0] + RND.LOG_DOUBLES * on[1] + 4 * on[2]
    assert (block is opt) == (not any(on))      # an option-free run hands opt_state itself back: no launch, no copy
    parts = a._log.split(block.clone())
    assert list(parts) == names
    for name, w in zip(names, want):
        assert torch.equal(parts[name], w), name
    if on[1]:      # the two RND parts are adjacent: together they are log_tail()'s layout
        assert torch.equal(torch.cat((parts["rnd_sums"], parts["rnd_block"])), RND.log_tail(a._rnd)) and RND.LOG_DOUBLES == 2 + L.RND_HEADER


def test_distillation_layout():
    bc = f64(51.0, 52.0)
    a = _alg(bc=bc)
    block = a._log.device()
    assert torch.equal(block, torch.cat((a.net.opt_state, bc)))
    parts = a._log.split(block)
    assert list(parts) == ["opt", "bc"] and torch.equal(parts["opt"], a.net.opt_state) and torch.equal(parts["bc"], bc)


def test_log_block_refuses_what_it_cannot_name():
    opt = ("opt", torch.zeros(3, dtype=torch.float64))
    with pytest.raises(AssertionError):
        LogBlock([opt, ("opt", torch.zeros(2, dtype=torch.float64))])      # a name twice
    with pytest.raises(AssertionError):
        LogBlock([opt, ("x", torch.zeros(2, dtype=torch.float32))])        # another dtype: torch.cat would promote
    with pytest.raises(AssertionError):
        LogBlock([opt]).split(torch.zeros(4, dtype=torch.float64))         # a block of another layout


def test_readers_against_the_offsets_they_replace():
    n = L.OPT_STATE
    # the mirror loss: sum / steps, behind opt_state
    a = _alg(mirror=f64(7.0, 2.0))
    block = a._log.device()
    assert mirror_loss_from(a, block) == 7.0 / 2.0 == float(block[n]) / max(float(block[n + 1]), 1.0)
    assert mirror_loss_from(_alg(mirror=f64(7.0, 0.0)), _alg(mirror=f64(7.0, 0.0))._log.device()) == 7.0      # no step: divides by 1
    assert smoothness_from(a, block) is None and rnd_log_from(a, block) is None
    # smoothness: the last four numbers; n = 0 divides by 1
    for sums, want in (((3.0, 5.0, 6.0, 0.0), dict(temporal=3.0, spatial=5.0, valid_fraction=6.0 / MB)),
                       ((3.0, 5.0, 6.0, 2.0), dict(temporal=1.5, spatial=2.5, valid_fraction=6.0 / (MB * 2.0)))):
        a = _alg(mirror=f64(7.0, 2.0), smooth=f64(*sums))
        block = a._log.device()
        assert smoothness_from(a, block) == want
        t, s, w, cnt = (float(x) for x in block[block.numel() - 4:])
        assert want == dict(temporal=t / max(cnt, 1.0), spatial=s / max(cnt, 1.0), valid_fraction=w / (MB * max(cnt, 1.0)))
        assert mirror_loss_from(a, block) == 3.5
    # RND: LOG_DOUBLES numbers ahead of the smoothness sums (or at the end without them)
    head = torch.zeros(L.RND_HEADER + 5, dtype=torch.float64)
    head[L.RND_ROWS], head[L.RND_SUM_INTRINSIC], head[L.RND_SUM_REWARDS], head[L.RND_WEIGHT_LAST], head[L.RND_STD] = 8.0, 2.0, 4.0, 0.75, 1.25
    want = {"Loss/rnd": 1.5, "Rnd/intrinsic_reward": 0.25, "Rnd/extrinsic_reward": 0.5, "Rnd/weight": 0.75, "Rnd/std": 1.25}
    for smooth in (None, f64(3.0, 5.0, 6.0, 2.0)):
        a = _alg(mirror=f64(7.0, 2.0), rnd=(f64(6.0, 4.0), head), smooth=smooth)
        block = a._log.device()
        got = rnd_log_from(a, block)
        assert got == want and list(got) == list(want) and a._rnd.last_log == want and a._rnd.last_loss == 1.5
        end = block.numel() - (4 if smooth is not None else 0)
        assert RND.log_from(SimpleNamespace(), block[end - RND.LOG_DOUBLES:end]) == want
        assert mirror_loss_from(a, block) == 3.5 and (smoothness_from(a, block) is None) == (smooth is None)
    # everything off
    a = _alg()
    block = a._log.device()
    assert mirror_loss_from(a, block) is None and smoothness_from(a, block) is None and rnd_log_from(a, block) is None
    # Distillation: sum / steps behind opt_state, and no mirror loss
    a = _alg(bc=f64(9.0, 4.0))
    block = a._log.device()
    assert Distillation.behavior_loss_from(a, block) == 9.0 / 4.0 == float(block[n]) / max(float(block[n + 1]), 1.0)
    assert mirror_loss_from(a, block) is None and a._options == ()


def test_log_scalars_order_and_conditions():
    rnd = _rnd(last_log={"Loss/rnd": 5.0, "Rnd/intrinsic_reward": 6.0, "Rnd/extrinsic_reward": 7.0, "Rnd/weight": 8.0, "Rnd/std": 9.0})
    a = SimpleNamespace(denoise_coef=0.5, last_denoise_loss=1.0,
                        _scalar_order=(_option(MirrorLoss, last=2.0), _option(Smoothness, last=dict(temporal=3.0, spatial=4.0, valid_fraction=1.0)), rnd))
    assert PPO.log_scalars(a) == [("Loss/denoise_mse", 1.0), ("Loss/mirror", 2.0), ("Loss/smooth_temporal", 3.0), ("Loss/smooth_spatial", 4.0),
                                  ("Loss/rnd", 5.0), ("Rnd/intrinsic_reward", 6.0), ("Rnd/extrinsic_reward", 7.0), ("Rnd/weight", 8.0), ("Rnd/std", 9.0)]
    a.denoise_coef, a._scalar_order, rnd.last_log = 0.0, (rnd,), None      # a value left behind, the other options off, RND on with nothing read yet
    assert PPO.log_scalars(a) == []
    a._scalar_order = ()
    assert PPO.log_scalars(a) == []


# ------------------------------------------------------------------------------------------------ PPO.check_setup
OK = dict(num_envs=64, num_transitions_per_env=8, num_mini_batches=2, num_actor_obs=5)
SMOOTH = dict(temporal_coef=1.0)


def _refused(message, **kw):
    with pytest.raises(ValueError, match=re.escape(message)):
        PPO.check_setup(**dict(OK, **kw))


def test_check_setup_refusals_and_their_messages():
    sym = object()
    PPO.check_setup(**OK)
    PPO.check_setup(64, 8, 2, 5)
    PPO.check_setup(**dict(OK, symmetry=sym, mirror_loss_coef=0.5, advantage_normalization="minibatch"))
    PPO.check_setup(**dict(OK, symmetry=sym, symmetry_augmentation=False, mirror_loss_coef=0.5, rnd=object()))      # the mirror loss without augmentation is fine
    PPO.check_setup(**dict(OK, rnd=object(), smoothness=SMOOTH, advantage_normalization="none"))
    PPO.check_setup(**dict(OK, symmetry=sym, smoothness=dict(temporal_coef=0.0, spatial_coef=0.0)))      # both coefficients 0: off
    PPO.check_setup(**dict(OK, num_envs=1, num_transitions_per_env=2, num_mini_batches=1, advantage_normalization="minibatch"))
    _refused("PPO.advantage_normalization='per-row': one of batch, minibatch, none", advantage_normalization="per-row")
    for bad in (-1.0, float("inf"), float("nan")):
        _refused("PPO.mirror_loss_coef=%r: must be finite and >= 0" % (bad,), mirror_loss_coef=bad, symmetry=sym)
    _refused("PPO.mirror_loss_coef=0.5 needs the mirror tables: set PPO.symmetry to a MirrorSpec", mirror_loss_coef=0.5)
    _refused("PPO.rnd runs on one rank (world size 2): the predictor's gradient has no exchange", rnd=object(), world=2)
    _refused("PPO.rnd does not support PPO.symmetry_augmentation: mirrored rows have no RND state (the mirror loss without augmentation is fine)",
             rnd=object(), symmetry=sym)
    _refused("PPO.smoothness runs on one rank (world size 2)", smoothness=SMOOTH, world=2)
    _refused("PPO.smoothness does not support PPO.symmetry (augmentation or mirror loss)", smoothness=SMOOTH, symmetry=sym, symmetry_augmentation=False)
    _refused("PPO.smoothness: unknown key lam (known: temporal_coef, spatial_coef, noise_std, noise_scale, seed)", smoothness=dict(lam=1.0))
    _refused("PPO.advantage_normalization='minibatch' needs minibatches of at least 2 rows (they have 1)", num_envs=1,
             num_transitions_per_env=3, num_mini_batches=3, advantage_normalization="minibatch")
    _refused("PPO.advantage_normalization='minibatch' needs minibatches of at least 2 rows (they have 1)", num_envs=1,      # doubled by the augmentation
             num_transitions_per_env=1, num_mini_batches=2, advantage_normalization="minibatch", symmetry=sym)


def test_check_setup_order_in_which_the_refusals_win():
    sym = object()
    small = dict(num_envs=1, num_transitions_per_env=1, num_mini_batches=1)
    _refused("one of batch, minibatch, none", advantage_normalization="x", mirror_loss_coef=-1.0, rnd=object(), smoothness=SMOOTH, world=2)
    _refused("must be finite and >= 0", mirror_loss_coef=-1.0, rnd=object(), smoothness=SMOOTH, world=2, advantage_normalization="minibatch", **small)
    _refused("needs the mirror tables", mirror_loss_coef=0.5, rnd=object(), smoothness=SMOOTH, world=2, advantage_normalization="minibatch", **small)
    _refused("PPO.rnd runs on one rank", rnd=object(), smoothness=SMOOTH, world=2, advantage_normalization="minibatch", **small)
    _refused("PPO.smoothness runs on one rank", smoothness=SMOOTH, world=2, advantage_normalization="minibatch", **small)
    _refused("PPO.rnd does not support PPO.symmetry_augmentation", rnd=object(), smoothness=SMOOTH, symmetry=sym)
    _refused("at least 2 rows", advantage_normalization="minibatch", **small)


def test_distillation_refuses_ahead_of_ppo():
    """Distillation.init_storage runs its own refusals first: each wins over a PPO.check_setup refusal of the same configuration, and all
    of them come before anything touches a device."""
    def alg(**kw):
        a = Distillation.__new__(Distillation)
        a._world, a.gradient_length, a.actor_critic = 1, 4, SimpleNamespace(num_actor_obs=5)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for message, kw in (("PPO.rnd does not support Distillation", dict(rnd=object(), advantage_normalization="x")),
                        ("PPO.smoothness does not support Distillation", dict(smoothness=SMOOTH, advantage_normalization="x")),
                        ("Distillation does not support PPO.symmetry / PPO.mirror_loss_coef", dict(mirror_loss_coef=-1.0)),
                        ("Distillation uses no advantages: advantage_normalization='x' must stay 'batch'", dict(advantage_normalization="x")),
                        ("Distillation needs a StudentTeacher policy, not SimpleNamespace", dict())):
        with pytest.raises(ValueError, match=re.escape(message)):
            alg(**kw).init_storage(64, 8, [5], [5], [3])
