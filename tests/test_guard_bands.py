"""The guard-band harness of tests/guard_common.py proved on CPU tensors: what tests/test_guard_bands_gpu.py relies
on when it calls a clean verify() proof that an entry point stayed inside its buffers.

  a. a store one element past a view, one element in front of it and one byte at the far edge of a band -- each made by plain torch
     through a deliberately over-wide view of the SAME allocation -- is reported with the buffer, the side and the offset;
  b. a clean writer passes; a reader that sums one element too many gets NaN (a consumed guard read poisons the result);
  c. carve honours align and skew for every dtype the GPU file carves;
  d. the Python mirrors of the header's size macros equal hgym._lib's, the header's text, and the library's own answers where it
     exports them (hgym_net_workspace_bytes, hgym_net_norm_layout, hgym_net_shadow_ld need no device)."""
import ctypes as C
import os
import re

import pytest
import torch

import guard_common as G

DTYPES = (torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool, torch.int16)


def _arena(n=3):
    return G.Arena("cpu", G.arena_bytes(*[4096] * n))


def _wide(arena, view):
    """(the whole allocation as bytes, byte offset of `view` in it): the over-wide view the errant stores go through."""
    return arena.raw, view.data_ptr() - arena.raw.data_ptr()


def _report(arena, what="writer"):
    with pytest.raises(G.GuardError) as e:
        arena.verify(what)
    return str(e.value)


def test_overrun_on_either_side_is_reported():
    a = _arena()
    first = a.carve((7, 5), torch.float32, name="first")
    x = a.carve((10, 3), torch.float32, name="x")
    last = a.carve(11, torch.int64, name="last")
    for t in (first, x, last):
        t.zero_()
    a.verify("zero fill")
    raw, off = _wide(a, x)
    wide = raw[off - 4:off + 4 * 31].view(torch.float32)       # one element more on either side
    # one element past the view
    wide[31] = 1.0
    msg = _report(a)
    assert msg.startswith("writer wrote outside its buffers") and msg.count("\n") == 1
    assert "x: behind band, bytes [%d, %d] relative to the buffer" % (120, 123) in msg and "4 changed" in msg     # 1.0f = 00 00 80 3f
    a.verify("the bands were refilled")
    # one element in front
    wide[0] = -2.5
    msg = _report(a)
    assert "x: front band, bytes [-4, -1] relative to the buffer" in msg and msg.count("\n") == 1
    # one byte at the far edge of either band
    raw[off + 120 + G.BAND - 1] = 0
    raw[off - G.BAND] = 7
    msg = _report(a)
    assert "x: front band, bytes [%d, %d] relative to the buffer, 1 changed" % (-G.BAND, -G.BAND) in msg
    assert "x: behind band, bytes [%d, %d] relative to the buffer, 1 changed" % (120 + G.BAND - 1, 120 + G.BAND - 1) in msg
    assert "first" not in msg and "last" not in msg
    # the neighbours' own bands are theirs
    raw2, off2 = _wide(a, last)
    raw2[off2 + 88] = 1
    assert "last: behind band, bytes [88, 88]" in _report(a)
    a.verify("clean again")
    assert torch.equal(x, torch.zeros(10, 3)) and int(last.sum()) == 0


def test_spare_band_at_the_end():
    """The behind-band of the last view is not the end of the allocation: one more band lies behind it."""
    a = G.Arena("cpu", G.arena_bytes(1000))
    v = a.carve(1000, torch.uint8)
    end = v.data_ptr() - a.raw.data_ptr() + 1000
    assert a.raw.numel() - end >= 2 * G.BAND
    with pytest.raises(MemoryError):
        a.carve(1000, torch.uint8)


def test_clean_writer_passes_and_consumed_guard_read_poisons():
    a = _arena(4)
    for dt in (torch.float32, torch.bfloat16, torch.float64):
        x = a.carve(33, dt)
        x.fill_(1.0)                                   # a clean writer
        a.verify("fill")
        raw, off = _wide(a, x)
        es = x.element_size()
        assert float(raw[off:off + 33 * es].view(dt).sum()) == 33.0               # a clean reader
        assert torch.isnan(raw[off:off + 34 * es].view(dt).sum())                 # one element too many
        assert torch.isnan(raw[off - es:off + 33 * es].view(dt).sum())
    i = a.carve(5, torch.int64)
    raw, off = _wide(a, i)
    assert int(raw[off + 40:off + 48].view(torch.int64)) == -1                    # an index read from a band points back into a band
    assert int(raw[off - 4:off].view(torch.int32)) == -1 and int(raw[off - 1]) == 255


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_carve_honours_align_and_skew(dtype):
    es = G.esize(torch.uint8 if dtype == torch.bool else dtype)
    a = G.Arena("cpu", G.arena_bytes(*[4096] * 10, align=4096))
    prev_end = a.raw.data_ptr()
    for align, skew in ((256, 0), (256, es), (16, 0), (4096, 0), (256, 4 if 4 % es == 0 else es), (64, 64 - es), (es, 0)):
        v = a.carve((3, 5), dtype, align=align, skew=skew)
        assert v.dtype == dtype and v.shape == (3, 5) and v.is_contiguous()
        assert v.data_ptr() % align == skew
        assert v.data_ptr() - prev_end >= G.BAND                 # a whole band in front, whatever the alignment gap
        prev_end = v.data_ptr() + 15 * es + G.BAND
        t = G.Plain("cpu").carve((3, 5), dtype, align=align, skew=skew)      # the twin's buffer: the same address class, the same bytes
        assert t.data_ptr() % align == skew and t.dtype == dtype and bool((t.view(torch.uint8) == 0xFF).all())
        assert bool((v.view(torch.uint8) == 0xFF).all())         # the contents start as guard bytes too
    p = a.place(torch.arange(15).reshape(3, 5).to(dtype), skew=es)
    assert torch.equal(p, torch.arange(15).reshape(3, 5).to(dtype)) and p.data_ptr() % 256 == es
    a.verify("carve and place")
    with pytest.raises(AssertionError):
        a.carve(4, torch.float32, skew=2)                        # not element-aligned


def test_size_macro_mirrors():
    from hgym import _lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hgym.h")).read()
    text = re.sub(r"\\\n", " ", header)
    text = re.sub(r"\s+", " ", text)
    for macro in ("#define HGYM_GAE_STATS_DOUBLES(n) (4 + 2 * (((n) + 15) / 16))",
                  "#define HGYM_ADV_MB_SCRATCH_DOUBLES(segments, seg_len) ((int64_t)(segments) * (3 + 2 * (((int64_t)(seg_len) + 1023) / 1024)))",
                  "#define HGYM_DIAG_SUMS 16", "#define HGYM_DIAG_ROWS_PER_PARTIAL 256",
                  "#define HGYM_DIAG_BLOCK_DOUBLES(total_rows) ((size_t)HGYM_DIAG_SUMS * (1 + ((size_t)(total_rows) + HGYM_DIAG_ROWS_PER_PARTIAL - 1) / HGYM_DIAG_ROWS_PER_PARTIAL))",
                  "#define HGYM_EVAL_SUMS 32", "#define HGYM_EVAL_ENVS_PER_PARTIAL 256", "#define HGYM_NUM_REWARDS 22",
                  "#define HGYM_EVAL_BLOCK_DOUBLES(n) ((size_t)HGYM_EVAL_SUMS * (1 + ((size_t)(n) + HGYM_EVAL_ENVS_PER_PARTIAL - 1) / HGYM_EVAL_ENVS_PER_PARTIAL) + (size_t)(2 + HGYM_NUM_REWARDS) * (size_t)(n))",
                  "#define HGYM_ROLLOUT_SCRATCH_HEADER_BYTES 512", "#define HGYM_ROLLOUT_DRAW_BYTES_PER_ENV 1000",
                  "#define HGYM_ROLLOUT_SCRATCH_BYTES(num_envs) (HGYM_ROLLOUT_SCRATCH_HEADER_BYTES + (size_t)HGYM_ROLLOUT_DRAW_BYTES_PER_ENV * (size_t)(num_envs))"):
        assert macro in text, macro
    for n in (1, 2, 15, 16, 17, 33, 255, 256, 257, 513, 1023, 1024, 1025, 4097):
        assert G.gae_stats_doubles(n) == L.gae_stats(n, "cpu").numel()
        assert G.diag_block_doubles(n) == L.diag_block_doubles(n)
        assert G.eval_block_doubles(n) == L.eval_block_doubles(n)
        assert G.rollout_scratch_bytes(n) == L.rollout_scratch_bytes(n)
        for s in (1, 3, 4, 7):
            assert G.adv_mb_scratch_doubles(s, n) == L.adv_mb_scratch_doubles(s, n)
    assert G.gae_stats_doubles(17) == 8 and G.adv_mb_scratch_doubles(4, 1025) == 28
    assert G.diag_block_doubles(257) == 48 and G.eval_block_doubles(257) == 96 + 24 * 257


def test_net_sizes_come_from_the_library():
    """What guard_net carves is what the library itself states, without a device: the workspace bytes, the norm block's size (its parts
    inside it) and the shadows' leading dimensions of the three nets of the GPU file."""
    import update_options_common as U
    from hgym import _lib as L, make_net_config, norm_layout
    for path in U.PATHS:
        no, npv, A, ah, ch = U.SHAPES[path]["net"]
        cfg = make_net_config(no, npv, A, ah, ch, "f32" if path == "f32-layer" else "bf16", 256, fused_activation=path == "bf16-fused")
        ws = int(L.lib.hgym_net_workspace_bytes(C.byref(cfg)))
        lay = norm_layout(cfg)
        assert ws > 0 and lay[L.NORM_BYTES] > 0
        parts = [lay[L.NORM_HEADER] + 64, lay[L.NORM_SUMS] + 8 * lay[L.NORM_SUMS_DOUBLES]] + \
                [lay[s + k] + w * K for k, K in enumerate((no, npv)) for s, w in ((L.NORM_MEAN, 8), (L.NORM_VAR, 8), (L.NORM_MEAN_F, 4), (L.NORM_SCALE_F, 4))]
        assert max(parts) <= lay[L.NORM_BYTES]
        ld = [int(L.lib.hgym_net_shadow_ld(C.byref(cfg), k)) for k in (0, 1)]
        assert ld == ([768, 256] if path == "bf16-fused" else [0, 0])
        assert G.net_arena_bytes(cfg, obs_norm=True) >= ws + lay[L.NORM_BYTES] + 16 * int(L.lib.hgym_net_param_count(C.byref(cfg)))


def test_phase_groups_by_hand():
    """guard_common.phase_groups at two shapes per entry, against grids worked out by hand from the launch sites."""
    P, F, FB, S, E = G.PhaseLaunch, G.FWD_SLOTS, G.FB_SLOTS, G.SIDE_SLOTS, G.ENV_SLOTS
    pg = G.phase_groups
    # hgym_policy_act: M = 33 -> two 32-row tiles per net, grid (2, 2); with the finaliser's row grid (2, 3), whose last row is silent
    assert pg("policy_act", dict(M=33, cus=256)) == [P(4, {0: [F], 1: [F], 2: [F], 3: [F]})]
    assert pg("policy_act", dict(M=33, cus=256, fin=True)) == [P(6, {0: [F], 1: [F], 2: [F], 3: [F]})]
    assert pg("policy_act", dict(M=33, cus=256, fin=True, generic=True)) == [P(4, {0: [F], 1: [F], 2: [F], 3: [F]})]
    # 256 CUs: 2 * ceil(4097 / 32) = 258 > 256 -> 64-row tiles, ceil(4097 / 64) = 65 per net; 4096 rows still fit in 32-row tiles
    big = pg("policy_act", dict(M=4097, cus=256))[0]
    assert big.groups == 130 and sorted(big.stamps) == list(range(130)) and len(big.slots()) == 130 * 7
    assert pg("policy_act", dict(M=4096, cus=256))[0].groups == 256
    # hgym_mlp_forward / a piece of hgym_critic_values: one net
    assert pg("mlp_forward", dict(M=1, cus=256)) == [P(1, {0: [F]})]
    assert pg("mlp_forward", dict(M=65, cus=256)) == [P(3, {0: [F], 1: [F], 2: [F]})]
    # the update tile: 64 rows; B = 200 -> 4 tiles, 2 or 3 nets
    assert pg("ppo_grad", dict(B=1, nets=2)) == [P(2, {0: [FB], 1: [FB]})]
    assert pg("ppo_grad", dict(B=200, nets=3))[0].groups == 12 and pg("ppo_grad", dict(B=65, nets=2))[0].groups == 4
    assert pg("bc_grad", dict(B=65)) == [P(2, {0: [FB], 1: [FB]})] and pg("bc_grad", dict(B=200))[0].groups == 4
    # the rollout step at N = 64: two columns, six groups; column 0 has its actor in row 0, column 1 in row 1
    assert pg("rollout_step", dict(N=64, form="first")) == [P(6, {0: [F], 3: [F], 2: [FB], 1: [FB], 4: [E], 5: [E]})]
    assert pg("rollout_step", dict(N=64, form="next")) == [P(6, {0: [F], 3: [F], 2: [FB], 1: [FB], 4: [E, (6, 7)], 5: [E, (6,)]})]
    assert pg("rollout_step", dict(N=64, form="deferred_first")) == [P(6, {0: [F], 1: [F], 4: [E], 5: [E]})]
    assert pg("rollout_step", dict(N=64, form="deferred_next")) == [P(6, {0: [F], 1: [F], 4: [E, (6, 7)], 5: [E, (6,)]})]
    # the 64-row layout at N = 320: ten columns; side jobs at columns 1, 3, 5, 7 and -- swapped -- 8; critic tiles at 0, 2, 4, 6 and 9
    assert [x for x in range(10) if G.rollout_side_column(x)] == [1, 3, 5, 7, 8]
    st = pg("rollout_step", dict(N=320, form="steady64"))[0]
    assert st.groups == 30
    non_actor = {x: ((1 - (x & 1)) * 10 + x) for x in range(10)}
    assert [x for x in range(10) if st.stamps[non_actor[x]] == [S]] == [1, 3, 5, 7, 8]
    assert [x for x in range(10) if st.stamps[non_actor[x]] == [FB]] == [0, 2, 4, 6, 9]
    assert all(st.stamps[(x & 1) * 10 + x] == [F] for x in range(10)) and st.stamps[20] == [E, (6, 7)] and st.stamps[29] == [E, (6,)]
    assert pg("rollout_step", dict(N=128, form="steady64"))[0].stamps[4 + 0] == [FB] and pg("rollout_eval_step", dict(N=64)) == []
