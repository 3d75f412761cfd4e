"""Shared by tests/test_guard_bands.py (CPU) and tests/test_guard_bands_gpu.py (-m gpu): guard bands around every buffer an entry point
of include/hgym.h is handed.  The library never allocates: every kernel writes through the caller's raw pointers,
and a store a few rows past M, or a size macro one chunk short, lands in the caching allocator's slack where no value test sees it.

  Arena       one uint8 allocation filled with 0xFF; carve() hands out views with BAND bytes of 0xFF in front and behind, verify()
              compares every band byte for byte.  All-ones is NaN as fp32 / bf16 / fp64, -1 as int32 / int64, 255 / true as uint8: a
              guard byte that is READ AND USED poisons the result (the callers assert finiteness), an index read from a band points
              back into a band.
  guard_net   a hgym.NetBuffers whose every buffer is an arena view of exactly the size the header states.
  guard_env   re-seats every own allocation of a hgym.EnvBuffers into an arena.
  *_doubles   Python mirrors of the header's size macros (tests/test_guard_bands.py holds them to hgym._lib's).

What the bands see: every store outside the stated ranges up to BAND bytes away, and every consumed load.  What they do not: a load of
band bytes that is masked out afterwards -- at the end of a real allocation that load would still be out of bounds; only a sanitizer
could see it."""
import ctypes as C
import math

import torch

# At least one full tile of the widest row any kernel here stages: 64 rows x 768 fp32 columns = 196 608 B; the next power of two.
BAND = 256 * 1024
FILL = 0xFF


def esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def arena_bytes(*nbytes, align=256):
    """Room for buffers of these byte sizes: each with its two bands and its alignment gap, and the spare band at the end."""
    return sum(int(n) + 2 * BAND + align for n in nbytes) + BAND


class GuardError(AssertionError):
    pass


class Arena:
    def __init__(self, device, nbytes):
        self.device = torch.device(device)
        self.raw = torch.full((int(nbytes),), FILL, dtype=torch.uint8, device=self.device)
        self._end = 0           # offset behind the last buffer's behind-band
        self.buffers = []       # (name, start, nbytes): byte offsets into raw

    def carve(self, shape, dtype, align=256, skew=0, name=None):
        """A contiguous view of `shape` whose byte address is skew (mod align); BAND guard bytes in front and behind, and one more
        spare band between the last behind-band and the end of the allocation.  The contents are 0xFF: the caller fills them."""
        shape = (shape,) if isinstance(shape, int) else tuple(int(s) for s in shape)
        store = torch.uint8 if dtype == torch.bool else dtype
        es = esize(store)
        assert 0 <= skew < align and skew % es == 0 and align % es == 0, (dtype, align, skew)
        n = math.prod(shape) * es
        start = self._end + BAND
        start += (skew - (self.raw.data_ptr() + start)) % align
        if start + n + 2 * BAND > self.raw.numel():
            raise MemoryError("arena of %d bytes is full (%d buffers): %d more needed" % (self.raw.numel(), len(self.buffers),
                                                                                      start + n + 2 * BAND - self.raw.numel()))
        self._end = start + n + BAND
        self.buffers.append((name or "buffer %d %s %s" % (len(self.buffers), tuple(shape), str(dtype).replace("torch.", "")), start, n))
        v = self.raw[start:start + n].view(store).view(shape)
        assert v.data_ptr() % align == skew
        return v.view(torch.bool) if dtype == torch.bool else v

    def place(self, tensor, **kw):
        """carve() + copy: a drop-in replacement for an existing tensor."""
        v = self.carve(tensor.shape, tensor.dtype, **kw)
        (v.view(torch.uint8) if tensor.dtype == torch.bool else v).copy_(tensor.view(torch.uint8) if tensor.dtype == torch.bool else tensor)
        return v

    def zeros(self, shape, dtype, **kw):
        v = self.carve(shape, dtype, **kw)
        v.view(torch.uint8).zero_()
        return v

    def _bands(self):
        for name, start, n in self.buffers:
            yield name, "front", start - BAND, start, start
            yield name, "behind", start + n, start + n + BAND, start

    def verify(self, what):
        """Every band byte against 0xFF: one device comparison per band, one read-back.  A mismatch raises GuardError naming, per band,
        the buffer, the side, the first and last changed byte offset RELATIVE TO THE BUFFER's first byte, and the count; the bands are
        refilled, so the next verify judges the next call alone."""
        bands = list(self._bands())
        if not bands:
            return
        counts = torch.stack([(self.raw[a:b] != FILL).sum() for _, _, a, b, _ in bands]).cpu().tolist()
        if not any(counts):
            return
        msgs = []
        for (name, side, a, b, start), c in zip(bands, counts):
            if c:
                bad = (self.raw[a:b] != FILL).nonzero().flatten()
                msgs.append("%s: %s band, bytes [%d, %d] relative to the buffer, %d changed"
                            % (name, side, int(bad[0]) + a - start, int(bad[-1]) + a - start, c))
                self.raw[a:b] = FILL
        raise GuardError("%s wrote outside its buffers:\n  %s" % (what, "\n  ".join(msgs)))


class Plain:
    """The unguarded twin's allocator: Arena's carve / place / zeros as ordinary torch tensors with the same initial bytes."""

    def __init__(self, device):
        self.device = torch.device(device)

    def carve(self, shape, dtype, align=256, skew=0, name=None):
        shape = (shape,) if isinstance(shape, int) else tuple(int(s) for s in shape)
        store = torch.uint8 if dtype == torch.bool else dtype
        n = math.prod(shape) * esize(store)
        raw = torch.full((n + 2 * align,), FILL, dtype=torch.uint8, device=self.device)
        start = (skew - raw.data_ptr()) % align      # the same address class as the guarded buffer: a kernel may pick its path by it
        v = raw[start:start + n].view(store).view(shape)
        assert v.data_ptr() % align == skew
        return v.view(torch.bool) if dtype == torch.bool else v

    place, zeros = Arena.place, Arena.zeros

    def verify(self, what):
        pass


# ------------------------------------------------------------------------------------------------ the header's size macros
def gae_stats_doubles(n):
    """HGYM_GAE_STATS_DOUBLES(n)."""
    return 4 + 2 * ((int(n) + 15) // 16)


def adv_mb_scratch_doubles(segments, seg_len):
    """HGYM_ADV_MB_SCRATCH_DOUBLES(segments, seg_len)."""
    return int(segments) * (3 + 2 * ((int(seg_len) + 1023) // 1024))


def diag_block_doubles(total_rows):
    """HGYM_DIAG_BLOCK_DOUBLES(total_rows)."""
    return 16 * (1 + (int(total_rows) + 255) // 256)


def eval_block_doubles(n):
    """HGYM_EVAL_BLOCK_DOUBLES(n)."""
    return 32 * (1 + (int(n) + 255) // 256) + (2 + 22) * int(n)


def rollout_scratch_bytes(num_envs):
    """HGYM_ROLLOUT_SCRATCH_BYTES(num_envs)."""
    return 512 + 1000 * int(num_envs)


# ------------------------------------------------------------------------------------------------ guarded NetBuffers / EnvBuffers
def net_arena_bytes(cfg, obs_norm=False):
    """arena_bytes for guard_net(cfg): four flat vectors, opt_state, the workspace and the norm block."""
    from hgym import _lib as L, norm_layout
    P = int(L.lib.hgym_net_param_count(C.byref(cfg)))
    sizes = [4 * P] * 3 + [4 * (P + 1), 8 * L.OPT_STATE, int(L.lib.hgym_net_workspace_bytes(C.byref(cfg)))]
    if obs_norm:
        sizes.append(norm_layout(cfg)[L.NORM_BYTES])
    return arena_bytes(*sizes)


def guard_net(cfg, arena, learning_rate=1e-5, obs_norm=None):
    """hgym.NetBuffers(cfg, arena.device, ...) with params, adam_m, adam_v, grads_ext (P + 1), opt_state, the workspace
    (hgym_net_workspace_bytes bytes, 256-aligned, zero-filled) and the norm block (layout[HGYM_NORM_BYTES] bytes) carved from the
    arena at exactly those sizes -- no + 256 padding -- and struct, views and sigma re-seated on them."""
    from hgym import NetBuffers, _lib as L

    class GuardedNet(NetBuffers):
        def __init__(self):
            super().__init__(cfg, arena.device, learning_rate=learning_rate, obs_norm=obs_norm)
            old, old_ws = self.params, self._ws_ptr
            z = lambda n, dt, name: arena.zeros(n, dt, name="net." + name)
            self.params, self.adam_m, self.adam_v = (z(self.P, torch.float32, k) for k in ("params", "adam_m", "adam_v"))
            self.grads_ext = z(self.P + 1, torch.float32, "grads_ext")
            self.grads = self.grads_ext[:self.P]
            self.opt_state = z(L.OPT_STATE, torch.float64, "opt_state")
            self.opt_state[L.OPT_LR] = learning_rate
            self.workspace = z(int(L.lib.hgym_net_workspace_bytes(C.byref(cfg))), torch.uint8, "workspace")
            self._ws_ptr = self.workspace.data_ptr()
            self.struct = L.Net(L.fptr(self.params), L.fptr(self.grads), L.fptr(self.adam_m), L.fptr(self.adam_v),
                                L.f64ptr(self.opt_state), C.c_void_p(self._ws_ptr))
            if self.obs_norm is not None:
                # no zero-fill: the header says hgym_net_norm_init writes every part that is read -- the block stays 0xFF until then
                self._norm_block = arena.carve(self.norm_layout[L.NORM_BYTES], torch.uint8, name="net.norm")
                self._norm_off = 0
                self.struct.norm = C.c_void_p(self._norm_block.data_ptr())
                eps, until = self.obs_norm
                L.check(L.lib.hgym_net_norm_init(C.byref(cfg), C.byref(self.struct), eps, -1 if until is None else until, self.stream()),
                        "hgym_net_norm_init")
            # the named views and sigma at the offsets the ordinary object gave them
            A = cfg.num_actions
            self.sigma = self.params[:A] if self.sigma.data_ptr() == old.data_ptr() else \
                self.workspace[self.sigma.data_ptr() - old_ws:self.sigma.data_ptr() - old_ws + 4 * A].view(torch.float32)
            for k, v in list(self.views.items()):
                o = (v.data_ptr() - old.data_ptr()) // 4
                self.views[k] = self.params[o:o + v.numel()].view_as(v)

    return GuardedNet()


ENV_TENSORS = ("_state", "episode_length", "counters", "obs_ring", "priv_ring", "episode_acc", "obs", "priv_obs", "rew", "reset", "time_out",
               "extras_time_outs", "extras_episode", "rew_alt", "reset_alt", "time_out_alt", "rollout_scratch", "log_cur", "log_stats",
               "reset_idx_mask", "reset_idx_ids", "reset_idx_rejected", "root", "dof_pos", "dof_vel", "dof_state", "contact", "rigid",
               "terrain_levels", "terrain_types", "terrain_origins", "height_samples", "height_points", "height_pose", "measured_heights",
               "command_range_x", "custom_rew", "custom_sums", "custom_acc", "extras_custom", "_l0_partial")


def env_arena_bytes(buf):
    own = [t for t in vars(buf).values() if torch.is_tensor(t) and t._base is None]
    return arena_bytes(*[t.numel() * t.element_size() for t in own], 2 * buf.N * 512 * 4)


def guard_env(buf, arena):
    """Every tensor attribute of a hgym.EnvBuffers that is its own allocation moves into the arena, contents kept; call it after the
    set_* options and before the first sim_struct / state_struct / out_struct.  The [C][N] field views are rebuilt on the moved state
    block, in L.ENV_STATE_FIELDS order; l0_partial's (2, N, 512) block is carved at exactly that size."""
    from hgym import _lib as L
    own = [k for k, t in vars(buf).items() if torch.is_tensor(t) and t._base is None]
    assert set(own) <= set(ENV_TENSORS), "EnvBuffers has tensors guard_env does not know: %s" % (set(own) - set(ENV_TENSORS))
    for k in own:
        setattr(buf, k, arena.place(getattr(buf, k), name="env." + k))
    off = 0
    for name, c in L.ENV_STATE_FIELDS:
        buf.f[name] = buf._state[off:off + c]
        off += c
    assert off == buf._state.shape[0]
    if buf._l0_partial is None:
        buf._l0_partial = arena.zeros((2, buf.N, 512), torch.float32, name="env._l0_partial")
    return buf


# ------------------------------------------------------------------------------------------------ the phase buffer's grids
# hgym_prof_phase_buffer (include/hgym.h): what every instrumented launch asks of the buffer and who stamps what,
# restated from the launch sites (csrc/hgym_net.hip, hgym_fwd_act.hip, hgym_fused.hpp, hgym_rollout.hip / .hpp) in plain Python.
FWD_SLOTS = (0, 1, 2, 3, 4, 5, 6)          # fwd_body: start, first chunk staged, first layer's products, its epilogue, layer 1, layer 2, head
FB_SLOTS = FWD_SLOTS + (7,)                # fb_body: + the end of the dZ chain
SIDE_SLOTS = (0, 1, 2, 7)                  # the rollout step's side-job workgroup: start, draws done, rows ahead stored, end
ENV_SLOTS = (0, 1, 2, 3, 4, 5)             # the rollout step's env part, in grid row 2's groups


class PhaseLaunch:
    """One phase_buffer(groups) request of the library: `groups` groups of 8 slots, and per group that anybody stamps the slot tuples of
    its writers, each in the writer's program order.  (Several kernel launches may share one request: the per-net launches of the
    any-activation kernels offset the pointer by the nets before them.)"""

    def __init__(self, groups, stamps):
        self.groups, self.stamps = int(groups), {int(g): [tuple(w) for w in ws] for g, ws in stamps.items()}
        assert all(0 <= g < self.groups for g in self.stamps)

    def __eq__(self, other):
        return (self.groups, self.stamps) == (other.groups, other.stamps)

    def __repr__(self):
        return "PhaseLaunch(%d, %r)" % (self.groups, self.stamps)

    def slots(self):
        """Every slot index (group * 8 + slot) that must change."""
        return sorted(g * 8 + s for g, ws in self.stamps.items() for w in ws for s in w)


def rollout_side_column(x):
    """64-row layout: is grid column x's non-actor workgroup the side-job workgroup of its pair of tiles (else their critic tile)?"""
    return ((x ^ (x >> 3)) & 1) != 0


def phase_groups(entry, shape):
    """[PhaseLaunch] of one call of `entry` at `shape` (a dict).  Entries and their shape keys:
      policy_act      M, cus, fin (hgym_policy_act_fin), generic (an activation other than ELU(1))
      mlp_forward     M, cus                 (which = 0, 1, 2 and every piece of hgym_critic_values: one net)
      ppo_grad        B, nets (2, or 3 with the fused auxiliary head)      (ELU(1), any activation, either value loss: the same grid)
      bc_grad         B
      rollout_step    N, form: "first" (inline, no finaliser), "next" (inline with the finaliser, 32-row layout: <1,0>, <1,1>, <1,1,1>),
                      "steady64" (<1,1,1,0,1>), "deferred_first", "deferred_next" (values = NULL, either activation form)
      rollout_eval_step  N                   (never instrumented)"""
    cdiv = lambda a, b: -(-int(a) // int(b))
    if entry in ("policy_act", "mlp_forward"):
        nets = 2 if entry == "policy_act" else 1
        M = int(shape["M"])
        bm = 64 if nets * cdiv(M, 32) > int(shape["cus"]) else 32          # forward_nets: 32-row tiles while they fit the chip in one round
        tiles = cdiv(M, bm)
        rows = nets + (1 if shape.get("fin") and not shape.get("generic") else 0)      # the finaliser's grid row stamps nothing
        return [PhaseLaunch(tiles * rows, {g: [FWD_SLOTS] for g in range(tiles * nets)})]
    if entry in ("ppo_grad", "bc_grad"):
        nets = int(shape.get("nets", 2)) if entry == "ppo_grad" else 1
        tiles = cdiv(shape["B"], 64)
        return [PhaseLaunch(tiles * nets, {g: [FB_SLOTS] for g in range(tiles * nets)})]
    if entry == "rollout_eval_step":
        return []
    if entry == "rollout_step":
        N, form = int(shape["N"]), shape["form"]
        assert N % 32 == 0
        X = N // 32
        stamps = {}
        for x in range(X):
            if form.startswith("deferred"):
                stamps[x] = [FWD_SLOTS]                                # the actor tile; grid row 1 is the finaliser's (or absent)
            else:
                actor_row = x & 1                                      # rows 0 and 1 trade places on odd columns
                stamps[actor_row * X + x] = [FWD_SLOTS]
                other = (1 - actor_row) * X + x
                if form == "steady64":
                    stamps[other] = [SIDE_SLOTS if rollout_side_column(x) else FB_SLOTS]      # 64-row critic tile: fwd_body's seven + the end
                else:
                    stamps[other] = [FB_SLOTS]                         # 32-row critic tile + its side jobs' end
            row2 = [ENV_SLOTS]                                          # written by the column's actor + env workgroup
            if form not in ("first", "deferred_first"):
                row2.append((6, 7) if x == 0 else (6,))               # the finaliser row's workgroup x; workgroup 0 is the finaliser
            stamps[2 * X + x] = row2
        return [PhaseLaunch(3 * X, stamps)]
    raise KeyError(entry)
