"""CPU-only: the first layer's k-step counts (csrc/hgym_fused.hpp: l0_ksteps).  The buffers of a first layer of width K stay padded to
whole 128-column chunks (KB = 4 ceil(K / 128) k-steps of 32 columns, NC = KB / 4 chunks); the loops run KR = ceil(K / 32) k-steps, the
last chunk nlast = KR - 4 (NC - 1) of them.  Read through the library's host-side test hook, which needs no device."""
import ctypes as C

import pytest

# K -> (KB, KR, NC, nlast), worked out by hand: K = 705 is 22 full k-steps + 1 column (k-step 22), chunk 5 holds k-steps 20..23
WANT = {
    1: (4, 1, 1, 1), 32: (4, 1, 1, 1), 33: (4, 2, 1, 2), 96: (4, 3, 1, 3),
    97: (4, 4, 1, 4), 128: (4, 4, 1, 4), 129: (8, 5, 2, 1), 160: (8, 5, 2, 1), 161: (8, 6, 2, 2), 219: (8, 7, 2, 3),
    224: (8, 7, 2, 3), 225: (8, 8, 2, 4), 256: (8, 8, 2, 4), 257: (12, 9, 3, 1), 705: (24, 23, 6, 3), 768: (24, 24, 6, 4),
}


def _hook():
    from hgym import _lib as L
    fn = L.lib.hgym_internal_l0_ksteps
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    return L, fn


@pytest.mark.parametrize("K", sorted(WANT))
def test_l0_ksteps_of_a_width(K):
    L, fn = _hook()
    out = (C.c_int32 * 4)()
    L.check(fn(None, 0, K, out), "hgym_internal_l0_ksteps")
    assert tuple(out) == WANT[K]
    KB, KR, NC, nlast = out
    assert 32 * (KR - 1) < K <= 32 * KR and 128 * (NC - 1) < K <= 128 * NC and KB == 4 * NC
    assert 1 <= nlast <= 4 and 4 * (NC - 1) + nlast == KR


@pytest.mark.parametrize("n_obs,n_priv", [(705, 219), (97, 161), (129, 224), (128, 225), (160, 97)])
def test_the_layout_runs_kr_and_keeps_every_buffer_padded(n_obs, n_priv):
    """What ws_layout fills for a net configuration: KR as above next to the padded KB, and the shadow's leading dimension
    (hgym_net_shadow_ld), which follows KB, where it was."""
    L, fn = _hook()
    from hgym import make_net_config
    from oracle import xbot_constants as XK
    cfg = make_net_config(n_obs, n_priv, 12, XK.ACTOR_HIDDEN, XK.CRITIC_HIDDEN, "bf16", 256)
    for which, K in ((0, n_obs), (1, n_priv)):
        out = (C.c_int32 * 4)()
        L.check(fn(C.byref(cfg), which, 0, out), "hgym_internal_l0_ksteps")
        assert tuple(out) == WANT[K], (which, K)
        assert L.lib.hgym_net_shadow_ld(C.byref(cfg), which) == 32 * out[0] == (K + 127) // 128 * 128


def test_l0_ksteps_refuses_bad_arguments():
    L, fn = _hook()
    out = (C.c_int32 * 4)()
    assert fn(None, 0, 0, out) != 0 and fn(None, 0, 705, None) != 0
