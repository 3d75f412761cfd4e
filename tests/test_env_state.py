"""CPU side of the env snapshot (EnvBuffers.state_dict / load_state_dict, LeggedRobot's guards, the checkpoint sidecar's name):

  * completeness: every buffer the three pointer structs of include/hgym.h name is either in EnvBuffers.state_entries() or in
    EnvBuffers.STATE_EXCLUDED with a reason -- a state field added later fails here instead of silently breaking an exact resume;
  * the round trip through torch.save / torch.load into a second buffer set, in place;
  * every refusal, with the field named;
  * the sidecar does not disturb helpers.get_load_path."""
import ctypes as C
import os
import types

import pytest
import torch

from hgym import EnvBuffers, default_env_config, _lib as L

N = 24


def _buffers(terrain=False, curriculum=False, custom=False, layout="soa", n=N, frame_stack=15, c_frame_stack=3):
    b = EnvBuffers(default_env_config(n, seed=3, frame_stack=frame_stack, c_frame_stack=c_frame_stack), "cpu", sim_layout=layout)
    if terrain:
        rows, cols, P = 3, 2, 5
        b.set_terrain(torch.rand(rows, cols, 3), torch.randint(0, rows, (n,)), torch.arange(n) % cols, 8.0, True,
                      height_samples=torch.zeros(40, 30, dtype=torch.int16), height_points=torch.rand(P, 3))
    if curriculum:
        b.set_command_curriculum([-0.3, 0.6], 1.5)
    if custom:
        b.set_custom_rewards([0, 7])
    return b


def _tensor_attrs(b):
    """name -> tensor for every tensor attribute of the buffer object (the [C][N] state fields are slices of `_state`)."""
    return {k: v for k, v in vars(b).items() if torch.is_tensor(v)}


def _owner(b, addr):
    """The attribute whose allocation holds device address `addr`."""
    hits = [k for k, t in _tensor_attrs(b).items() if t.data_ptr() <= addr < t.data_ptr() + max(t.numel() * t.element_size(), 1)]
    assert len(hits) == 1, (hex(addr), hits)
    return hits[0]


def _pointers(struct):
    """(field name, address) of every non-null pointer field of a ctypes struct, nested HgymStrided bases included."""
    out = []
    for name, typ in struct._fields_:
        v = getattr(struct, name)
        if isinstance(v, L.Strided):
            v, name = v.base, name + ".base"
        if typ is C.c_void_p:
            if v:
                out.append((name, int(v)))
        elif isinstance(v, C._Pointer):
            a = C.cast(v, C.c_void_p).value
            if a:
                out.append((name, a))
    return out


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("terrain,curriculum,custom", [(False, False, False), (True, True, True), (True, False, False), (False, True, True)])
def test_every_struct_pointer_is_state_or_excluded_with_a_reason(layout, terrain, curriculum, custom):
    b = _buffers(terrain, curriculum, custom, layout)
    b.log_sink = True                                   # (so that out_struct names the log sink's buffers too)
    b.l0_partial(0)
    listed = {name if name != "state" else "_state" for name, t, _ in b.state_entries() if t is not None}
    assert all(isinstance(r, str) and len(r) > 10 for r in b.STATE_EXCLUDED.values())
    assert not listed & set(b.STATE_EXCLUDED), "a buffer is both state and excluded"
    seen = set()
    for struct in (b.state_struct(), b.sim_struct(), b.out_struct(), b.out_struct(alt=True)):
        for field, addr in _pointers(struct):
            owner = _owner(b, addr)
            seen.add(owner)
            assert owner in listed or owner in b.STATE_EXCLUDED, \
                "%s.%s points into EnvBuffers.%s, which is neither in state_entries() nor in STATE_EXCLUDED" % (type(struct).__name__, field, owner)
    # the converse: everything listed is something the kernels can reach, and every tensor attribute is accounted for
    assert listed <= seen, listed - seen
    assert set(_tensor_attrs(b)) <= listed | set(b.STATE_EXCLUDED), set(_tensor_attrs(b)) - listed - set(b.STATE_EXCLUDED)
    # every row of the state block is in it through `state`
    assert b._state.shape[0] == sum(c for _, c in L.ENV_STATE_FIELDS)
    opt = b.state_meta()["optional"]
    assert opt == dict(terrain_levels=terrain, measured_heights=terrain, command_range_x=curriculum, custom_sums=custom, custom_acc=custom,
                       extras_custom=custom)


def _fill_distinct(b, seed):
    g = torch.Generator().manual_seed(seed)
    for k, (name, t, _) in enumerate(b.state_entries()):
        if t is None:
            continue
        if t.dtype == torch.bool:
            t.copy_(torch.rand(t.shape, generator=g) < 0.5)
        elif t.is_floating_point():
            t.copy_(torch.rand(t.shape, generator=g, dtype=torch.float64).to(t.dtype) + k)
        else:
            t.copy_(torch.randint(1000 * k + 1, 1000 * k + 999, t.shape, generator=g).to(t.dtype))


@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("options", [False, True])
def test_round_trip_through_a_file_in_place(tmp_path, layout, options):
    a, b = _buffers(options, options, options, layout), _buffers(options, options, options, layout)
    _fill_distinct(a, 1)
    for _, t, _ in b.state_entries():
        if t is not None:
            t.zero_()
    sd = a.state_dict()
    for name, t, _ in a.state_entries():                # clones, not views
        assert (name in sd) == (t is not None)
        if t is not None:
            assert sd[name].data_ptr() != t.data_ptr() and sd[name].dtype == t.dtype and sd[name].shape == t.shape
    torch.save(dict(env=sd, iterations_done=3), str(tmp_path / "envstate_2.pt"))
    back = torch.load(str(tmp_path / "envstate_2.pt"), map_location="cpu")["env"]
    assert back["meta"] == a.state_meta() and back["meta"]["version"] == EnvBuffers.STATE_FORMAT
    ptrs = {k: t.data_ptr() for k, t in _tensor_attrs(b).items()}
    structs = [bytes(b.state_struct()), bytes(b.sim_struct()), bytes(b.out_struct())]
    b.load_state_dict(back)
    assert {k: t.data_ptr() for k, t in _tensor_attrs(b).items()} == ptrs, "load_state_dict re-allocated a buffer"
    assert [bytes(b.state_struct()), bytes(b.sim_struct()), bytes(b.out_struct())] == structs
    for name, t, _ in b.state_entries():
        if t is not None:
            src = dict((n, x) for n, x, _ in a.state_entries())[name]
            assert t.dtype == src.dtype and t.shape == src.shape and torch.equal(t, src), name
    sd2 = b.state_dict()
    assert sd2["meta"] == sd["meta"] and all(torch.equal(sd2[k], sd[k]) for k in sd if k != "meta")
    # friction, base mass and the origins are rows of the state block: the original env's draws survive
    for f in ("friction", "body_mass", "env_origins"):
        assert torch.equal(b.f[f], a.f[f]) and float(b.f[f].abs().min()) > 0


def test_snapshot_into_caller_buffers_and_current_rows():
    a = _buffers()
    _fill_distinct(a, 2)
    host = a.state_host_buffers(pin=False)
    assert set(host) == {n for n, t, _ in a.state_entries() if t is not None}
    cur = (torch.full_like(a.obs, 7.0), torch.full_like(a.priv_obs, 9.0))       # the rows live elsewhere (a rollout storage slot)
    sd = a.state_dict(out=host, current=cur)
    assert all(sd[k] is host[k] for k in host)
    assert torch.equal(sd["obs"], cur[0]) and torch.equal(sd["priv_obs"], cur[1]) and torch.equal(sd["state"], a._state)
    b = _buffers()
    dst = (torch.zeros_like(b.obs), torch.zeros_like(b.priv_obs))
    obs0 = b.obs.clone()
    b.load_state_dict(sd, current=dst)
    assert torch.equal(dst[0], cur[0]) and torch.equal(dst[1], cur[1]) and torch.equal(b.obs, obs0)


def test_every_refusal_names_the_field():
    a = _buffers()
    sd = a.state_dict()
    keep = _buffers()
    _fill_distinct(keep, 5)
    before = keep.state_dict()

    def refused(target, bad, word):
        with pytest.raises(ValueError, match=word):
            target.load_state_dict(bad)

    refused(_buffers(n=N + 8), sd, "num_envs")
    refused(_buffers(frame_stack=4), sd, "frame_stack")
    refused(_buffers(c_frame_stack=2), sd, "c_frame_stack")
    refused(_buffers(layout="aos"), sd, "sim_layout")
    refused(keep, dict(sd, meta=dict(sd["meta"], version=EnvBuffers.STATE_FORMAT + 1)), "version")
    refused(keep, {k: v for k, v in sd.items() if k != "meta"}, "meta")
    refused(_buffers(terrain=True), sd, "terrain_levels")
    refused(keep, _buffers(terrain=True).state_dict(), "terrain_levels")
    refused(_buffers(curriculum=True), sd, "command_range_x")
    refused(keep, _buffers(curriculum=True).state_dict(), "command_range_x")
    refused(_buffers(custom=True), sd, "custom_sums")
    refused(keep, _buffers(custom=True).state_dict(), "custom_sums")
    refused(keep, {k: v for k, v in sd.items() if k != "obs_ring"}, "obs_ring")
    refused(keep, dict(sd, counters=sd["counters"][:3]), "counters")
    refused(keep, dict(sd, rew=sd["rew"].double()), "rew")
    after = keep.state_dict()                           # a refused load writes nothing
    assert all(torch.equal(after[k], before[k]) for k in before if k != "meta")


def test_env_refuses_between_the_launches_of_a_step():
    """LeggedRobot.state_dict / load_state_dict while a postponed finaliser is pending or a fused rollout is open (the guard both
    call; tests/test_exact_resume_gpu.py raises them on a live env)."""
    from humanoid.envs.base.legged_robot import LeggedRobot
    for what in ("state_dict", "load_state_dict"):
        LeggedRobot._refuse_mid_step(types.SimpleNamespace(), what)
        LeggedRobot._refuse_mid_step(types.SimpleNamespace(_pending_fin=None, _in_rollout=False), what)
        with pytest.raises(ValueError, match="_pending_fin"):
            LeggedRobot._refuse_mid_step(types.SimpleNamespace(_pending_fin=(1, 2, 3), _in_rollout=False), what)
        with pytest.raises(ValueError, match="_in_rollout"):
            LeggedRobot._refuse_mid_step(types.SimpleNamespace(_pending_fin=None, _in_rollout=True), what)


def test_sidecar_name_and_get_load_path(tmp_path):
    from humanoid.algo import OnPolicyRunner
    from humanoid.utils.helpers import get_load_path
    run = tmp_path / "Oct16_10-00-00_"
    run.mkdir()
    for it in (0, 2):
        model = str(run / ("model_%d.pt" % it))
        side = OnPolicyRunner.env_state_path(model)
        assert os.path.basename(side) == "envstate_%d.pt" % it and os.path.dirname(side) == str(run)
        for p in (model, side):
            open(p, "wb").close()
    assert get_load_path(str(tmp_path), checkpoint=-1) == str(run / "model_2.pt")
    assert get_load_path(str(tmp_path), checkpoint=0) == str(run / "model_0.pt")
    for name in ("sync.pt", "model_final.pt", "my_model.pt"):
        assert "model" not in os.path.basename(OnPolicyRunner.env_state_path(str(run / name))), name
