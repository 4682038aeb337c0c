"""Moving buildings crossed with the features that read the same device records through other kernels: counted handles
(env_kernel_counted, safety_scan_counted_kernel, building_rows_counted_kernel), set_drone_counts in mid-run,
CityRoutePlanner.redraw, rvo3d_rvo_vel_city along a flown trajectory and post_train with safety=True in both loops.

Everything is compared bit for bit with what the suite already pins: the twin design of tests/test_gpu_building_motion.py
(a handle M whose sets are moved on the device against a handle H that is given the numpy reference's positions through
set_env_buildings before every step), CityRoutePlanner.sample_numpy / plan_numpy, tests/rvo_city_ref.py and safety_numpy.
The inputs and the CPU flights are in tests/moving_city_case.py; tests/test_moving_city_host.py recounts the figures below.

1. The twin on counted handles: the sets, patrols and actions of test_gpu_building_motion.inputs, 25 steps, both autoreset
settings.  Counts (cycled over the envs; env e has set e % 3), what set_drone_counts puts in force at step 8, None at 16:

    N x E      at the start               from step 8
    8 x 21     (8, 1, 3, 5, 2, 8, 7)      every fourth env takes its neighbour's count
    64 x 6     (64, 33, 48, 1, 63, 2)     (64, 48, 20, 30, 63, 2)
    100 x 3    (1, 100, 33)               (65, 20, 33)

The CPU oracle (every env alone at its count, one OracleEnv per env and step with that step's list, plain steps + reset of
the drones that are done or have finished) gave, over the 25 steps: done flags that differ from the same run with the
sets left standing inside the envs of B / of C, bclear entries (safety_numpy) that differ.  The GPU run must reach half of
each figure (moving_city_case.floor: glibc's and ocml's asin / acos may move a drone on a knife edge), here and below:

    N x E      B flags   C flags   bclear
    8 x 21      57       197       1965
    64 x 6      98       333       3574
    100 x 3    103       288       2810

2. Re-draws: CityRoutePlanner(RouteSampler(map of the sets, min_sep 1, min_len 10, seed 7)), P = 6, a plain and a counted
handle at 8 x 21 and 64 x 6; redraw(M, 1) before step t1 = 3, redraw(M, 2, env_mask) before step t2 = 6, the mask leaves
the last env of every set out (and at 8 x 21 also the first).  Since the start / since t1 the reference trajectory has:
buildings of B, of C in another cell, leg flips (envs 0 - 2); and the restatement round the start positions gives another
route than round the positions of step t for that many live drones of B envs / of C envs inside the mask (on the GPU the
device's routes must equal the restatement round the positions of step t and are then compared with the one round the
start):

    N x E     before t1     before t2      plain: t1, t2            counted: t1, t2
    8 x 21    5, 11, 1      6, 16, 5       43 / 54, 31 / 40         28 / 33, 20 / 24
    64 x 6    2, 13, 1      2, 16, 5       56 / 121, 35 / 61        45 / 48, 21 / 46

3. The city controller flown by the evaluator's rules: E 4, N 65, counts (65, 64, 1, 33), nb_max 6, building counts
(6, 5, 0, 6), map (20, 16, 8), radius 0.4, 12 steps, episodes of at most 6 steps; per env 5, 3, 0, 4 records arrive and
flip within the 12 moves.  The whole loop on the CPU (rvo_city_ref over ref.drone_side, the oracle's step) gave: drones x
steps in tier 1 / 2 / 3, candidates blocked only because their building moves, gated records on the arrival branch,
records of the first two episodes per env whose minimum bclear differs from the evaluation without the motion:

    tier 1   tier 2   tier 3   moving only   arrival   records
    1827     17       112      1369          1107      6

4. The second pass of rvo_city_body: tests/test_gpu_rvo_city.py::test_the_second_pass_across_waves_and_tiles (its figures
are in that test's docstring).

Deliberately wrong variants these tests catch, by construction: device_buildings() returning the start positions - part 2
compares the device's routes with the restatement round trajectory()[t], which differs from the one round the start in the
drones counted above (tried once with device_buildings() patched inside redraw: "step 3: re-draw, waypoints" fails); an
evaluator that scans before the buildings move - part 3 (b) compares every record with the fold of safety_numpy on the
positions after that step's move, and on the CPU the fold over the positions before the move changes all six records of
the envs that have buildings (tests/test_moving_city_host.py asserts at least four)."""
import functools

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, BuildingMotion
from rvo3d_amd.policy.post_train import post_train
from rvo3d_amd.safety import safety_numpy
import moving_city_case as mc
import rvo_city_ref as ref
from test_gpu_building_motion import (OUT_KEYS, RADIUS, T, assert_handles_equal, assert_live_positions,
                                      assert_readers_equal, bits_equal, host, inputs, trajectory)

pytestmark = pytest.mark.gpu

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_ghosts_are_zeros(env, counts, what):
    if counts is None:
        return
    ghost = np.arange(env.N)[None, :] >= np.asarray(counts)[:, None]
    for k in OUT_KEYS:
        assert not np.any(host(getattr(env, k))[ghost].view(np.uint8)), f"{what}: ghost rows of {k}"


# ---- 1. / 2. the twin ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def run(N, E, autoreset, mode):
    """M (motion attached) against H (the reference's positions before every step) over T steps; mode "counts": counted
    handles, set_drone_counts at CHANGE_AT and RESTORE_AT, beside S whose sets stand still; "plain" / "counted": re-draws
    before the steps redraw_steps() on a plain / a counted handle.  Returns the tallies the tests assert on."""
    redraw = mode != "counts"
    world, ends, speed = inputs(N, E)
    if redraw:
        world = mc.redraw_world(N, E)
    pos, legs = trajectory(N, E)
    counts = None if mode == "plain" else mc.start_counts(N, E)
    build = lambda: BatchedDroneEnv(world.with_drone_counts(counts), radius=RADIUS)
    M, H = build(), build()
    envs = [M, H] + ([] if redraw else [build()])
    S = None if redraw else envs[2]
    motion = BuildingMotion(ends, speed, dt=1.0)
    M.attach_building_motion(motion)
    if counts is not None:
        assert "env_kernel_counted" in M.kernel_name()
    for x in envs:
        x.observe()
    assert_handles_equal(M, H, "start")
    of_set = [np.arange(s, E, 3) for s in range(3)]
    tally = dict(done=0, flags=[0, 0, 0], bclear_diff=0, stale=[])
    steps = dict(zip(mc.redraw_steps(N, E), mc.DRAWS)) if redraw else {}
    pl = mc.planner()
    for t in range(T):
        what = f"{N}x{E} {mode} autoreset={autoreset} step {t}"
        if not redraw and t in (mc.CHANGE_AT, mc.RESTORE_AT):
            counts = mc.counts_at(N, E, t)
            for x in envs:
                x.set_drone_counts(counts)
                x.observe()
            assert ("env_kernel_counted" in M.kernel_name()) == (counts is not None)
            # the counts call has not disturbed the records: they are where the reference is, and M still equals H
            assert M._motion is motion and M.device_buildings()[0] is motion.buildings
            assert_live_positions(motion, world, pos[t], what + ": after set_drone_counts")
            assert np.array_equal(host(motion.leg), legs[t]), what + ": leg after set_drone_counts"
            assert_handles_equal(M, H, what + ": after set_drone_counts")
            assert_readers_equal(M, H, what + ": after set_drone_counts")
        if t in steps:
            draw, first = steps[t], t == min(steps)
            mask = None if first else mc.redraw_mask(E)
            rows = np.ones(E, bool) if mask is None else mask
            before = [host(r) for r in M.routes()]
            ret = pl.redraw(M, draw, None if mask is None else dev(mask))
            got = [host(r) for r in ret]
            want = mc.restated_redraw(N, E, t, draw)
            for g, w, name in zip(got, want, ("waypoints", "n_points", "unplaced", "blocked")):
                assert g.dtype == w.dtype and np.array_equal(g[rows], w[rows]), f"{what}: re-draw, {name}"
            live = np.ones((E, N), bool) if counts is None else np.arange(N)[None, :] < counts[:, None]
            wp, npts = (host(r) for r in M.routes())
            new = live & rows[:, None]
            assert np.array_equal(wp[new], want[0][new]) and np.array_equal(npts[new], want[1][new]), what + ": routes()"
            assert np.array_equal(wp[~new], before[0][~new]) and np.array_equal(npts[~new], before[1][~new]), \
                what + ": the envs outside the mask (and the ghosts) keep their routes"
            stale = mc.restated_redraw(N, E, 0, draw)
            diff = ((wp != stale[0]).any(axis=(2, 3)) | (npts != stale[1])) & new
            tally["stale"].append((int(diff[of_set[1]].sum()), int(diff[of_set[2]].sum())))
            H.set_routes(ret[0].clone(), ret[1].clone(), None if mask is None else dev(mask))
            for x in envs:
                x.observe()
            assert_handles_equal(M, H, what + ": after the re-draw")
        a = dev(mc.actions(N, E, t, counts))
        H.set_env_buildings(pos[t + 1], world.building_counts)
        for x in envs:
            x.step(a, autoreset=autoreset)
        assert_handles_equal(M, H, what)
        assert_ghosts_are_zeros(M, counts, what)
        bld, cnt = M.device_buildings()
        assert bld is motion.buildings and np.array_equal(host(cnt), world.building_counts)
        assert_live_positions(motion, world, pos[t + 1], what)
        assert np.array_equal(host(motion.leg), legs[t + 1]), what + ": leg"
        done = host(M.done).astype(bool)
        tally["done"] += int(done.sum())
        if S is not None:
            static = host(S.done).astype(bool)
            for s in range(3):
                tally["flags"][s] += int((done[of_set[s]] != static[of_set[s]]).sum())
        if not autoreset:
            assert_readers_equal(M, H, what)
            if S is not None:
                tally["bclear_diff"] += int((host(M.safety()[1]) != host(S.safety()[1])).sum())
            for x in envs:
                x.reset_drones(x.done | x.finish)
                x.observe()
            assert_handles_equal(M, H, what + ", after the resets")
    assert M.error_flags() == H.error_flags()
    for x in envs:
        x.close()
    print(f"{N}x{E} {mode} autoreset={autoreset}: {tally}")
    return tally


@pytest.mark.parametrize("N,E", mc.SHAPES)
@pytest.mark.parametrize("autoreset", [True, False])
def test_counted_handles_moved_on_the_device_equal_set_from_the_host(N, E, autoreset):
    """Every output and state key after each of 25 steps, behind plain steps also safety() and building_rows(k=4), the
    ghost rows zeros; set_drone_counts at step 8 (ups, downs and unchanged envs) and None at step 16 with the motion
    attached: M stays H, and the motion's records and leg stay the reference trajectory's."""
    c1, c2 = mc.start_counts(N, E), mc.changed_counts(N, E)
    assert 1 in c1 and N in c1 and (c2 > c1).any() and (c2 < c1).any() and (c2 == c1).any()
    assert N != 100 or (c1 <= 36).any()
    tally = run(N, E, autoreset, "counts")
    assert tally["done"] > 0, tally


@pytest.mark.parametrize("N,E", mc.SHAPES)
def test_the_motion_matters_to_counted_handles(N, E):
    tally = run(N, E, False, "counts")
    floor = [mc.floor(x) for x in mc.TWIN_FIGURES[(N, E)]]
    assert tally["flags"][0] == 0 and tally["flags"][1] >= floor[0] and tally["flags"][2] >= floor[1], tally
    assert tally["bclear_diff"] >= floor[2], tally


@pytest.mark.parametrize("N,E", mc.REDRAW_SHAPES)
@pytest.mark.parametrize("mode", ["plain", "counted"])
@pytest.mark.parametrize("autoreset", [True, False])
def test_redraws_go_round_the_buildings_where_they_are_now(N, E, mode, autoreset):
    """redraw(M) before steps t1 and t2 (the second with an env_mask): waypoints, n_points, unplaced and blocked are the
    restatement's round trajectory()[t] in the masked envs, the others keep their routes, H gets the same arrays through
    set_routes and the twin goes on to step 25; the routes differ from the restatement round the start positions."""
    tally = run(N, E, autoreset, mode)
    assert len(tally["stale"]) == 2, tally
    for got, cpu in zip(tally["stale"], mc.REDRAW_FIGURES[(N, E, mode)]):
        assert got[0] >= mc.floor(cpu[0]) and got[1] >= mc.floor(cpu[1]), (tally, cpu)


# ---- 3. the city controller and the evaluator along a flown trajectory -------------------------------------------------------

def city_env(moving=True):
    sc = mc.city_scene()
    env = BatchedDroneEnv(sc.world, radius=mc.CITY_RADIUS)
    motion = None
    if moving:
        motion = BuildingMotion(sc.ends, sc.speed, dt=1.0)
        env.attach_building_motion(motion)
    return env, motion


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def hand_loop():
    """(a): 12 steps of rvo_vel_city -> step -> safety by the evaluator's rules (an env whose episode ends - a drone done,
    CITY_EP_LEN steps, all finished - is reset; the buildings are not), every step against rvo_city_ref, the reference
    trajectory and safety_numpy.  Returns the tallies and, per env, the minimum bclear of its episodes."""
    import collections
    sc = mc.city_scene()
    pos, legs = mc.city_trajectory()
    E, N, counts, bcounts = mc.CITY_E, mc.CITY_N, mc.CITY_COUNTS, mc.CITY_BCOUNTS
    live = np.arange(N)[None, :] < counts[:, None]
    live_b = np.arange(mc.CITY_NB)[None, :] < bcounts[:, None]
    env, motion = city_env()
    env.reset(); env.observe()
    tally = collections.Counter()
    ep_len = np.zeros(E, np.int64)
    bmin, ended_all = np.full((mc.CITY_STEPS, E), np.inf), np.zeros((mc.CITY_STEPS, E), bool)
    for t in range(mc.CITY_STEPS):
        what = f"step {t}"
        st = env.get_state()
        p, v = host(st["pos"]), host(st["vel"])
        out, diag = env.rvo_vel_city(diagnostics=True, **mc.CITY_KW)
        bld, leg = host(motion.buildings), host(motion.leg)
        assert bits_equal(bld[live_b], pos[t][live_b]) and bits_equal(bld[~live_b], sc.bld0[~live_b]), what + ": records"
        assert np.array_equal(leg, legs[t]), what + ": leg"
        args = (p, v, mc.CITY_RADIUS, bld, u64(diag["live_mask"]), u64(diag["cone_mask"]), host(diag["tc_min"]),
                host(env.des_vel()))
        kw = dict(dt=1.0, counts=counts, building_counts=bcounts, **mc.CITY_KW)
        want = ref.rvo_city_ref(*args, motion=(sc.ends, sc.speed, leg), **kw)
        assert np.array_equal(u64(diag["live_mask"]), want["live_mask"]), what
        assert np.array_equal(u64(diag["blocked_mask"]), want["blocked_mask"]), what
        assert np.array_equal(host(diag["n_gated"]), want["n_gated"]), what
        assert np.array_equal(host(diag["tier"]), want["tier"]), what
        assert np.array_equal(bits(host(out)), bits(want["out_vel"])), what
        assert not host(out)[~live].any() and not want["tier"][~live].any(), what + ": ghost rows"
        for k in (1, 2, 3):
            tally[f"tier{k}"] += int((want["tier"] == k).sum())
        still = ref.rvo_city_ref(*args, motion=None, **kw)
        tally["moving_only"] += sum(bin(int(x)).count("1") for x in (want["blocked_mask"] & ~still["blocked_mask"]).ravel())
        for e in range(E):
            tally["arrival_gated"] += mc.arrivals(p[e, :counts[e]], bld[e, :bcounts[e]], e, leg[e])
        _, _, _, done, _, fin = env.step(out)
        assert bits_equal(host(motion.buildings)[live_b], pos[t + 1][live_b]), what + ": records behind the step"
        after = host(env.get_state()["pos"])
        got = [host(x) for x in env.safety()]
        num = safety_numpy(after, mc.CITY_RADIUS, sc.world.map_size, 0.5, counts=counts, buildings=pos[t + 1],
                           building_counts=bcounts)
        for g, w, name in zip(got, num, ("sep", "bclear", "wall", "near_pairs")):
            assert g.dtype == w.dtype and np.array_equal(g, w), f"{what}: safety {name}"
        bmin[t] = num[1].min(axis=1)
        ep_len += 1
        ended = host(done).astype(bool).any(1) | (ep_len == mc.CITY_EP_LEN) | (host(fin).astype(bool) | ~live).all(1)
        ended_all[t] = ended
        env.reset(dev(ended)); env.observe()
        ep_len[ended] = 0
    env.close()
    print("hand loop:", dict(tally))
    return dict(tally), mc.fold_episodes(bmin, ended_all)


def test_city_controller_along_a_flown_trajectory():
    """(a) blocked_mask, n_gated, tier and out_vel against rvo_city_ref at every one of 12 steps, without exemptions, from
    the device's own live_mask / cone_mask / tc_min / des_vel(), the state read back before the step, motion.buildings and
    (ends, speed, motion.leg); motion.buildings against the reference trajectory; safety() against safety_numpy."""
    flips = mc.city_flips()
    assert (flips[mc.CITY_BCOUNTS > 0] >= 2).all(), flips
    tally, episodes = hand_loop()
    for k in ("tier1", "tier2", "tier3", "moving_only", "arrival_gated"):
        assert tally[k] >= mc.floor(mc.CITY_FIGURES[k]), (k, tally)
    assert all(len(ep) >= 2 for ep in episodes), episodes


@functools.lru_cache(maxsize=None)
def evaluate(fused, moving=True):
    """post_train(policy_type="rvo_city", safety=True, poll_every=1), two episodes per env -> (result, records sorted
    by (step, env) as the host loop appends them, per env its records' minimum bclear)."""
    env, _ = city_env(moving)
    E = mc.CITY_E
    pt = post_train(env, num_episodes=2 * E, max_ep_len=mc.CITY_EP_LEN, fused=fused, safety=True, rvo=dict(mc.CITY_KW),
                    poll_every=1, inf_print=False)
    result = pt.policy_test(policy_type="rvo_city")
    keys = ("rec_min_sep", "rec_min_bclear", "rec_min_wall", "rec_near")
    per_env = None
    if fused:
        per_env = np.asarray(pt.records["rec_min_bclear"])
        order = np.lexsort((np.repeat(np.arange(E), 2), np.asarray(pt.records["rec_step"]).reshape(-1)))
        rec = {k: np.asarray(pt.records[k]).reshape(-1)[order] for k in keys}
    else:
        rec = {k: np.asarray(pt.safety_records[k]).reshape(-1) for k in keys}
    env.close()
    return result, rec, per_env


def test_both_evaluator_loops_agree_in_a_moving_city():
    """(b) the host loop and the fused loop on a fresh env and motion each: equal results and equal safety records, and
    every record's minimum bclear is the fold of (a)'s safety_numpy bclear over that episode's steps - positions that
    depend on the global step from the second episode on -, bit for bit.  The records differ from the evaluation without
    the motion."""
    r_host, s_host, _ = evaluate(False)
    r_fused, s_fused, per_env = evaluate(True)
    assert r_host == r_fused and r_host["episodes"] == 2 * mc.CITY_E, (r_host, r_fused)
    for k in s_host:
        assert s_host[k].shape == s_fused[k].shape == (2 * mc.CITY_E,), k
        assert np.array_equal(s_host[k], s_fused[k]), (k, s_host[k], s_fused[k])
    _, episodes = hand_loop()
    for e in range(mc.CITY_E):
        assert np.array_equal(per_env[e], np.array(episodes[e][:2])), (e, per_env[e], episodes[e][:2])
    _, _, static = evaluate(True, False)
    differ = int((static != per_env).sum())
    print("records that differ from the evaluation without the motion:", differ)
    assert differ >= mc.floor(mc.CITY_FIGURES["records"]), (per_env, static)
