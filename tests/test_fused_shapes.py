"""CPU-only: which bf16 nets take the fused kernels (csrc/hgym_fused.hpp), decided on the host before anything launches.

fused_supported() / fused_aux_supported() (csrc/hgym_net.hip) accept a family of layer widths; of those, only the shapes whose
mlp_fb_kernel tile fits in a workgroup's 160 KiB of LDS can train on that path.  hgym_net_shadow_ld is pure host code (it reports
the bf16 input shadow, which exists on the fused path only), so the decision is pinned here over the whole family against a
Python restatement of the kernel's LDS arithmetic."""
import ctypes as C

import pytest

from oracle import xbot_constants as K

LDS_LIMIT = 160 * 1024
WIDTHS = [128 * i for i in range(1, 7)]          # second / third hidden widths fused_supported() accepts: multiples of 128 up to 768


def _cdiv(a, b):
    return -(-a // b)


def fb_lds_bytes(hidden, head):
    """Dynamic LDS of one mlp_fb_kernel tile (64 rows) of a net with hidden widths `hidden` (3) and `head` outputs:
    hgym_fused.hpp fb_lds_bytes = fused_lds_p(n, 64) + fused_lds_q(n, 64) + fused_lds_bias(n) + fb_lds_extra(n)."""
    n0, n1, n2 = hidden
    p = 64 * max(n0, n2) * 2                                        # fused_lds_p        (hgym_fused.hpp:73)
    q = max(2 * 64 * 128 * 2, 64 * n1 * 2)                          # fused_lds_q        (hgym_fused.hpp:76-79, FUSED_CHUNK = 128)
    bias = (n0 + n1 + n2 + 16 * _cdiv(head, 16) + 16) * 4           # fused_lds_bias     (hgym_fused.hpp:75)
    lin = 64 * 2 * 4 if head == 1 else (64 * 40 * 4 if head <= 12 else 0)      # fb_lds_lin (hgym_fused.hpp:953-954)
    extra = 64 * 64 * _cdiv(head, 32) + 4 * 32 * 4 + 64 * n2 * 2 + 256 + lin    # fb_lds_extra (hgym_fused.hpp:955)
    return p + q + bias + extra


def _cfg(ah, ch, A=12, aux=None):
    from hgym import make_net_config
    if aux is None:
        return make_net_config(705, 219, A, ah, ch, "bf16", 4096)
    hidden, out = aux
    return make_net_config(705, 219, A, ah, ch, "bf16", 4096, aux_hidden=hidden, aux_out=out, aux_target_offset=219 - out)


def _shadow_ld(cfg):
    from hgym import _lib as L
    return int(L.lib.hgym_net_shadow_ld(C.byref(cfg), 0)), int(L.lib.hgym_net_shadow_ld(C.byref(cfg), 1))


def _fused(ah, ch, A=12):
    a, c = _shadow_ld(_cfg(ah, ch, A))
    assert (a > 0) == (c > 0), (ah, ch, a, c)        # one flag for both nets
    return a > 0


def _ws_bytes(cfg):
    from hgym import _lib as L
    return int(L.lib.hgym_net_workspace_bytes(C.byref(cfg)))


def test_restatement_reproduces_the_xbot_l_figures():
    # XBot-L: actor 133 504 B, critic 157 568 B; and three shapes the family accepts that do not fit
    assert fb_lds_bytes(K.ACTOR_HIDDEN, 12) == 133504
    assert fb_lds_bytes(K.CRITIC_HIDDEN, 1) == 157568
    assert fb_lds_bytes([768, 256, 128], 12) == 167296
    assert fb_lds_bytes([768, 256, 256], 1) == 174464
    assert fb_lds_bytes([512, 768, 128], 96) == 199360


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_fused_exactly_when_the_update_tile_fits(which):
    """Every trunk shape fused_supported() accepts, for the actor (head 12) and the critic (head 1), the other net held at a shape that
    fits: fused (shadow_ld > 0) exactly when the restated LDS budget is <= 160 KiB."""
    other = [256, 128, 128]
    head = 12 if which == "actor" else 1
    assert fb_lds_bytes(other, 1 if which == "actor" else 12) <= LDS_LIMIT
    wrong, over = [], 0
    for n0 in (256, 512, 768):
        for n1 in WIDTHS:
            for n2 in WIDTHS:
                h = [n0, n1, n2]
                fits = fb_lds_bytes(h, head) <= LDS_LIMIT
                over += not fits
                got = _fused(h, other) if which == "actor" else _fused(other, h)
                if got != fits:
                    wrong.append((h, fb_lds_bytes(h, head), got))
    assert not wrong, wrong
    assert over == (92 if which == "actor" else 83)      # of the 108: the refusals are real, not a corner


@pytest.mark.parametrize("A", [1, 5, 10, 12])
def test_actor_heads_below_twelve_follow_the_same_budget(A):
    """num_actions 1..12 all take the 40-float loss-input rows (fb_lds_lin): the decision does not depend on A."""
    for h in ([512, 256, 128], [512, 384, 128], [768, 256, 128], [512, 768, 256]):
        assert _fused(h, [256, 128, 128], A) == (fb_lds_bytes(h, A) <= LDS_LIMIT), (h, A)


def test_aux_head_fused_exactly_when_its_tile_fits(monkeypatch):
    """The denoiser head's family (first width 512, head 17..96) on the XBot-L trunk: its own fused layout (the workspace differs from the
    one HGYM_NO_FUSED_AUX forces) exactly when its update tile fits; the trunk stays fused either way."""
    wrong = []
    n_fit = n_over = 0
    for n1 in WIDTHS:
        for n2 in WIDTHS:
            for out in range(17, 97):
                cfg = _cfg(K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, aux=([512, n1, n2], out))
                fits = fb_lds_bytes([512, n1, n2], out) <= LDS_LIMIT
                n_fit += fits
                n_over += not fits
                fused_bytes = _ws_bytes(cfg)
                monkeypatch.setenv("HGYM_NO_FUSED_AUX", "1")
                generic_bytes = _ws_bytes(cfg)
                monkeypatch.delenv("HGYM_NO_FUSED_AUX")
                assert fused_bytes > 0 and generic_bytes > 0
                if (fused_bytes != generic_bytes) != fits:
                    wrong.append(([512, n1, n2], out, fb_lds_bytes([512, n1, n2], out)))
                assert min(_shadow_ld(cfg)) > 0
    assert not wrong, wrong
    assert n_fit > 0 and n_over > 0


def test_named_points(monkeypatch):
    assert _fused(K.ACTOR_HIDDEN, K.CRITIC_HIDDEN)                       # XBot-L
    assert _shadow_ld(_cfg(K.ACTOR_HIDDEN, K.CRITIC_HIDDEN)) == (768, 256)
    assert _fused([256, 256, 256], [256, 256, 256])                      # ActorCritic's own default (the reference's)
    assert not _fused([768, 256, 128], [768, 256, 128])                  # 167 296 B: the critic's widths on the actor
    assert not _fused(K.ACTOR_HIDDEN, [768, 256, 256])                   # 174 464 B
    assert not _fused([768, 768, 768], [768, 768, 768])
    assert _shadow_ld(_cfg([768, 256, 128], [768, 256, 128])) == (0, 0)
    # the XBot-L DWL head [512, 256, 128] -> 73 keeps its fused layout; [512, 768, 128] -> 96 (199 360 B) does not
    dwl = _cfg(K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, aux=([512, 256, 128], 73))
    big = _cfg(K.ACTOR_HIDDEN, K.CRITIC_HIDDEN, aux=([512, 768, 128], 96))
    fused = {"dwl": _ws_bytes(dwl), "big": _ws_bytes(big)}
    monkeypatch.setenv("HGYM_NO_FUSED_AUX", "1")
    assert _ws_bytes(dwl) != fused["dwl"]
    assert _ws_bytes(big) == fused["big"]
    monkeypatch.delenv("HGYM_NO_FUSED_AUX")
    assert min(_shadow_ld(dwl)) > 0 and min(_shadow_ld(big)) > 0
