"""CPU-only: the planted edge table of env_edges_common.py through the host emulation of the env kernel source, in every chain form
(the monolithic chain, the split phase sequence, the chain by roles in both lane orders), against the fp32 oracle and against the
float64 restatement of the step.  The `-m gpu` twin is test_env_edges_gpu.py."""
import ctypes as C

import pytest
import torch

import env_common as EC
import env_edges_common as EE


def test_the_table_reaches_both_sides_of_every_edge():
    """The census, counted from the float64 reference over the three passes: every named edge has a case on each side; the table's
    length is fixed; the fp32 oracle and the float64 reference take the same side everywhere (asserted while building)."""
    assert len(EE.CASES) == EE.NUM_CASES and len({n for n, _, _ in EE.CASES}) == EE.NUM_CASES
    built, census = EE.build_all()
    for edge, sides in census.items():
        print(edge, sides)
        assert all(n > 0 for n in sides.values()), (edge, sides)
    assert len(census) == 34
    for pname, b in built.items():
        print("%s pass: the fp32 oracle's distance from the float64 reference, in units of the fp32 bar" % pname)
        for k, v in b["oracle_distance"].items():
            print("  %-28s %.4f" % (k, v))


@pytest.mark.parametrize("split", [0, 1, 2, 3])
@pytest.mark.parametrize("layout,epb,nthreads", [("soa", 8, 64), ("aos", 16, 256), ("soa", 32, 512), ("aos", 32, 256)])
@pytest.mark.parametrize("pass_name", ["ones", "default", "signed"])
def test_planted_edges_host(pass_name, layout, epb, nthreads, split):
    """N = 154: 99 cases among 55 ordinary envs; blocks of 8 / 16 / 32 envs all leave a ragged last block.  Every pass in both layouts."""
    be = EC.HostBackend(envs_per_block=epb, nthreads=nthreads, split=split)
    EE.run_table(be, pass_name, sim_layout=layout)
    if split == 0 and epb == 8:
        EE.report_errors(be.name, pass_name)


@pytest.mark.parametrize("split", [0, 1, 2, 3])
@pytest.mark.parametrize("rows_ahead,hist", [(False, False), (True, False), (False, True)])
def test_clipped_frames_travel_through_the_ring_host(split, rows_ahead, hist):
    """The planted step and 15 more: the frames beyond the observation clip go through every older slot of the stacked rows (and,
    rows_ahead, through the rows written one step ahead: HgymEnvOut.obs_ahead / priv_ahead).  hist: the older frames are copied by
    hist_load / hist_store, the register-prefetched form the device kernels run, instead of stack_old."""
    be = EC.HostBackend(envs_per_block=16, nthreads=256, split=split, hist=hist)
    EE.run_table(be, "default", sim_layout="soa", rows_ahead=rows_ahead, more_steps=15)


def test_generic_options_edges_host():
    """Terrain map, terrain curriculum, height measurements and the command curriculum (monolithic chain only): base beyond each edge
    and corner of the height map, the yaw-quaternion norm floor, level promotion / demotion either side of their distance bars, out of
    the top row and at level 0, the command curriculum either side of its bar and at its cap.  Both layouts; the census of the three
    passes together has a case on every side."""
    total = {}
    for pass_name in EE.GENERIC_PASSES:
        for layout in ("soa", "aos"):
            C = EE.run_generic(EC.HostBackend(envs_per_block=8, nthreads=64), pass_name, layout)
        for edge, sides in C.items():
            for side, n in sides.items():
                total.setdefault(edge, {}).setdefault(side, 0)
                total[edge][side] += n
    want = {"height map px": 3, "height map py": 3, "height map corner": 1, "yaw quaternion norm": 2, "level promotion": 2, "level demotion": 2,
            "level range": 3, "command curriculum": 2, "command curriculum cap": 2}
    print(total)
    assert {e: len(s) for e, s in total.items()} == want and all(n > 0 for s in total.values() for n in s.values()), total
    assert len(EE.GENERIC_CASES) == EE.NUM_GENERIC_CASES


def test_whole_blocks_host():
    """N = 160 = 5 whole blocks of 32: the fast staging paths (16-byte row copies) instead of the ragged element-wise ones."""
    be = EC.HostBackend(envs_per_block=32, nthreads=256, split=1)
    EE.run_table(be, "ones", sim_layout="soa", nfill=61)


@pytest.mark.parametrize("split", [0, 1, 2, 3])
def test_state_side_edges_fused_step_host(split):
    """The fused step of the kernel source (its own Philox sim frame) with the state-side subset of the edges planted, in every chain
    form: env_edges_common.run_fused_state_edges."""
    import synth_common as SC
    from hgym import EnvBuffers, default_env_config
    from oracle import synth_env_oracle as S
    from oracle.xbot_env_oracle import XBotEnvOracle
    N, epb, nthreads, seed = 100, 16, 256, 0x5EED0EDE
    be = EC.HostBackend(envs_per_block=epb, nthreads=nthreads, split=split)
    g = torch.Generator().manual_seed(N + 1)
    cfg = default_env_config(N, seed=seed)
    buf = EnvBuffers(cfg, "cpu")
    buf.f["friction"].copy_((0.1 + 1.9 * torch.rand(N, generator=g)).view(1, N))
    buf.f["body_mass"].copy_((10.0 + 10.0 * torch.rand(N, generator=g)).view(1, N))
    sim, st, out = buf.sim_struct(), buf.state_struct(), buf.out_struct()
    be.lib.hc_env_step_ex(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(out), None, None, 1, 0, epb, nthreads, 0)      # prime
    o0 = XBotEnvOracle(N, frictions=buf.view("friction").clone(), body_mass=buf.view("body_mass").clone())
    S.synth_prime(o0, seed)
    SC.compare(buf, o0, "prime", [0])

    def step(a):
        ad = a.clone().contiguous()
        be.lib.hc_env_step_ex(C.byref(cfg), C.byref(sim), C.byref(st), C.byref(out), None, C.cast(ad.data_ptr(), C.POINTER(C.c_float)),
                              0, 1, epb, nthreads, split)
    counts, reached, flips = EE.run_fused_state_edges(buf, step, lambda: None, g, seed, 18)
    SC.report("kernel source on the host, fused step with planted state-side edges (split=%d) vs oracle, N=%d: %s; sim-side edges "
              "reached (information): %s" % (split, N, counts, reached), flips)
    assert counts["push"] == 1 and counts["timeout"] >= 3
