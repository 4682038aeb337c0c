"""The float32 pair filters of the fused env step (stage G and stage X1, csrc/rvo3d_pairs.hpp) at their error bands:
the worlds of tests/filter_edge_cases.py - pairs within 1e-8 .. 1e-3 of the gate, the touch surfaces, v . rel = 0 and
the cone's centi-radian tie, on maps up to 4000 m (and one of 1e6 m), at the far corner, the near corner, outside the
map and on both sides of the cmax bypass - against the CPU oracle, with the parity tests' own bar: done / info /
finish / vo_count / reset_mask bit-exact, observations and rewards f32-exact, the error word equal to the oracle's,
knife-edge accounting through test_gpu_parity.Tally (names filter_edges/...).

tests/test_filter_edges_host.py shows on the CPU that every constructed decision changes the oracle's output and that
a float32 filter without bands misreads the pairs.  Every instantiation of the filters is met and checked by name:
eight envs per wave (8 x 16), the padded 32-lane ring (24 x 6), one env per wave (64 x 4), the padded 128 ring and the
256 ring with gate_words_shared (100 x 3, 256 x 2), the generic kernel (300 x 2), and the counted handle with unequal
drone counts (ghost lanes beside the pairs).  observe() rounds reach stage G and x1_pairs<., ZERO = true>; step()
rounds, with and without auto-reset, the general action path, on positions after the move.
"""
import numpy as np
import pytest
import torch

import filter_edge_cases as fe
from rvo3d_amd import BatchedDroneEnv, World
from test_gpu_parity import Tally, close, eq_nan, resync_from_oracle

pytestmark = pytest.mark.gpu

CASES = [(s, m, c) for s in fe.SHAPES for m in fe.MAPS for c in fe.CONFIGS if c != "reset"]
RESET_CASES = [(s, m) for s in fe.SHAPES for m in fe.MAPS if m != fe.CONTROL]


def _pair(case):
    world = World(case.waypoints, case.n_points, case.map_size)
    if case.counts is not None:
        world = world.with_drone_counts(case.counts)
    env = BatchedDroneEnv(world, neighbors_num=fe.NM, env_train=case.env_train, radius=case.radius,
                          priority=case.priority)
    name = env.kernel_name("step_autoreset")
    assert name.endswith(case.kernel.format(t="true" if case.env_train else "false")), name
    return env, fe.RefBatch(case)


def _call(env, ref, tl, what, actions=None, autoreset=False):
    """observe() (actions None) or one step on both sides, compared at the parity tests' bar; the error word too.
    Returns the oracle's vo_count and reset mask."""
    dom0, nan0 = ref.domain_count, ref.nan_count
    rm = None
    if actions is None:
        obs, cnt = env.observe()
        ro, rcnt = ref.observe()
        tl.begin(ref.margin())
    else:
        obs, cnt, rew, done, info, fin = env.step(torch.from_numpy(actions).cuda(), autoreset=autoreset)
        ro, rcnt, rr, rdone, ri, rf, rm = ref.step(actions, autoreset)
        tl.begin(ref.margin())
        if autoreset:
            tl.check(f"reset_mask {what}", env.reset_mask.cpu().numpy() == rm)
        r = rew.cpu().numpy()
        tl.check(f"done {what}", done.cpu().numpy() == rdone)
        tl.check(f"info {what}", info.cpu().numpy() == ri)
        tl.check(f"finish {what}", fin.cpu().numpy() == rf)
        tl.check(f"reward {what}", close(r, rr))
        tl.check(f"reward f32-exact {what}", eq_nan(r, rr.astype(np.float32)))
    o = obs.cpu().numpy()
    tl.check(f"vo_count {what}", cnt.cpu().numpy() == rcnt)
    tl.check(f"obs {what}", close(o, ro))
    tl.check(f"obs f32-exact {what}", eq_nan(o, ro.astype(np.float32)))
    diverged = tl.end().any()
    flags = env.error_flags()
    if not diverged:  # (an exempt sample that differed may have met - or missed - such an event)
        assert (flags & 1) == (1 if ref.nan_count > nan0 else 0), what
        assert bool(flags & 2) == (ref.domain_count > dom0), what
    resync_from_oracle(env, ref, tl)
    return rcnt, rm


@pytest.mark.parametrize("shape,map_name,config", CASES)
def test_filters_at_their_error_bands(shape, map_name, config):
    case = fe.Case(shape, map_name, config)
    env, ref = _pair(case)
    tl = Tally(f"filter_edges/{shape}_{map_name}_{config}", case.E)
    rows = resets = 0
    for k, rd in enumerate(case.rounds):
        st = case.full_state(rd)
        env.set_state(**st); ref.set_state(**st)
        rcnt, rm = _call(env, ref, tl, f"round {k} {rd.mode}/{rd.bucket}/{rd.where}",
                         None if rd.mode == "observe" else rd.actions, rd.autoreset)
        rows += int(rcnt.sum())
        resets += 0 if rm is None else int(rm.sum())
    assert not tl.dropped.any()
    env.close()
    rec = tl.finish(rounds=len(case.rounds), vo_rows=rows, resets=resets)
    print(rec)
    assert rows > 0, rec


@pytest.mark.parametrize("shape,map_name", RESET_CASES)
def test_words_on_file_after_resets_at_the_gate(shape, map_name):
    """regate_resets (one-wave workgroups; a full stage G elsewhere): the first step resets the partner to a start
    waypoint at a gate or touch distance -+ d from i, the second step's reward sweep reads the stage-G words the first
    one filed."""
    case = fe.Case(shape, map_name, "reset")
    env, ref = _pair(case)
    tl = Tally(f"filter_edges/{shape}_{map_name}_reset", case.E)
    resets = 0
    for k, rd in enumerate(case.rounds):
        st = case.full_state(rd)
        env.set_state(**st); ref.set_state(**st)
        _, rm = _call(env, ref, tl, f"round {k} first step", rd.actions, True)
        resets += int(rm.sum())
        _call(env, ref, tl, f"round {k} second step", rd.actions2, rd.autoreset)
    assert not tl.dropped.any()
    env.close()
    rec = tl.finish(rounds=len(case.rounds), resets=resets)
    print(rec)
    assert resets > 0, rec
