"""The non-vacuity figures of tests/test_gpu_moving_city.py and of the second-pass case of tests/test_gpu_rvo_city.py,
recounted on the CPU (tests/moving_city_case.py): the tables in those docstrings are moving_city_case's constants, the
floors the GPU tests assert are half of them, and this module counts them again so that neither can rot.  No GPU needed.

What is made of numpy's correctly rounded operations, plain Python floats and the CPU oracle's geometry alone is
recounted exactly; the closed loop of part 3 goes through numpy's asin / acos (ref.drone_side), so it may be off by the
few drones another libm moves across a knife edge: within 10 % of the table, and never below twice the floor."""
import numpy as np
import pytest

import moving_city_case as mc


@pytest.mark.parametrize("N,E", mc.SHAPES)
def test_counts_of_the_twin(N, E):
    c1, c2 = mc.start_counts(N, E), mc.changed_counts(N, E)
    assert 1 in c1 and N in c1 and any(c % 4 for c in c1 if c not in (1, N))
    assert (c2 > c1).any() and (c2 < c1).any() and (c2 == c1).any() and c2.min() >= 1 and c2.max() <= N
    assert N != 100 or (c1 <= 36).any()   # a second wave of ghosts alone
    for s in range(3):                    # every building set sees a fleet that is cut down, before or after the change
        assert (c1[s::3] < N).any() or (c2[s::3] < N).any()


@pytest.mark.parametrize("N,E", mc.SHAPES)
def test_the_motion_matters_to_counted_fleets(N, E):
    """Part 1: done flags inside the envs of B and of C, and bclear, against the same flight with the sets left standing."""
    got = mc.twin_figures(N, E)
    print(N, E, got)
    assert got == mc.TWIN_FIGURES[(N, E)]
    assert all(x >= 2 * mc.floor(x) >= 2 for x in got)
    dm, _ = mc.cpu_flight(N, E, True)
    ds, _ = mc.cpu_flight(N, E, False)
    assert not (dm != ds)[:, 0::3].any()   # set A is empty: nothing to differ by


@pytest.mark.parametrize("N,E", mc.REDRAW_SHAPES)
def test_redraw_steps_and_stale_routes(N, E):
    """Part 2: before t1 and between t1 and t2 a building of B and one of C changes its cell and a record flips leg; the
    restatement round the start positions gives other routes, in drones of B and of C envs, at both re-draws."""
    t1, t2 = mc.redraw_steps(N, E)
    assert (t1, t2) == mc.REDRAW_STEPS[(N, E)] and 0 < t1 < t2 < mc.T
    changes = (mc.changes_between(N, E, 0, t1), mc.changes_between(N, E, t1, t2))
    assert changes == mc.REDRAW_CHANGES[(N, E)] and min(min(c) for c in changes) >= 1
    m = mc.redraw_mask(E)
    for s in range(3):
        assert m[s::3].any() and not m[s::3].all()
    for mode, counts in (("plain", None), ("counted", mc.start_counts(N, E))):
        got = tuple(mc.redraw_figures(N, E, counts))
        print(N, E, mode, got)
        assert got == mc.REDRAW_FIGURES[(N, E, mode)]
        assert all(x >= 2 * mc.floor(x) >= 2 for pair in got for x in pair)
    for t, draw in zip((t1, t2), mc.DRAWS):   # the comparison covers detours and failures
        wp, npts, unp, blocked = mc.restated_redraw(N, E, t, draw)
        assert (npts > 2).any() and blocked.any()


def test_city_scene_and_its_flight():
    """Part 3: the scene's shape, its arrivals, and the evaluator's loop on the CPU: tiers 1, 2 and 3, candidates blocked
    only because their building moves, gated records on the arrival branch, records the motion changes."""
    sc = mc.city_scene()
    assert sc.world.shape == (4, 65, 2) and sc.bld0.shape == (4, 6, 4)
    assert sc.world.drone_counts.tolist() == [65, 64, 1, 33] and sc.world.building_counts.tolist() == [6, 5, 0, 6]
    assert tuple(sc.world.map_size) == (20.0, 16.0, 8.0)
    flips = mc.city_flips()
    assert tuple(flips) == mc.CITY_FLIPS and (flips[mc.CITY_BCOUNTS > 0] >= 2).all()
    live_b = np.arange(mc.CITY_NB)[None, :] < mc.CITY_BCOUNTS[:, None]
    assert (sc.speed[live_b] == 0).any() and (sc.speed[live_b] > 0).any()   # static records beside the patrols
    got = dict(zip(("tier1", "tier2", "tier3", "moving_only", "arrival_gated", "records"), mc.city_figures()))
    print(got)
    for k, table in mc.CITY_FIGURES.items():
        assert got[k] >= 2 * mc.floor(table) >= 2, (k, got)
        assert abs(got[k] - table) <= max(0.1 * table, 2), (k, got)
    for moving in (True, False):
        assert all(len(ep) >= 2 for ep in mc.cpu_city_flight(moving)["episodes"])
    # an evaluator that scanned before the buildings move would write other records
    m = mc.cpu_city_flight(True)
    early = sum(int(a != b) for e in range(mc.CITY_E) for a, b in zip(m["episodes"][e][:2], m["episodes_early"][e][:2]))
    print("records an early scan changes:", early)
    assert early >= 4


def test_second_pass_scene():
    """Part 4: tier-3 lanes with two distinct tb beyond lane 64, a winner whose least tb comes from record 192 (and a lane
    whose velocity changes when the second tile is left out), an env with a wave that needs no second pass."""
    sc = mc.second_pass_scene()
    assert (sc.E, sc.N) == (2, 130) and sc.bld0.shape[1] == mc.PASS_TILE + 1 == 193 and sc.cnt[0] == 193
    assert (sc.drone_counts < sc.N).any() and mc.PASS_KW["acceler"] == 1.0
    got = mc.second_pass_cpu()
    print(got)
    assert got == mc.PASS_FIGURES
    assert got["distinct_64"] >= 20 and got["from_192"] >= 2 and got["first_tile_differs"] >= 2 and got["mixed_envs"] >= 1


def test_table_of_the_existing_cases():
    """The tier-3 figures of two CASES of test_gpu_rvo_city.py, whose floors that test now asserts."""
    got = mc.table_figures()
    assert got == mc.TABLE_FIGURES
    assert got["the wave seam, two tiles"][0] >= 60 and got["the wave seam, two tiles"][1] >= 8   # the floors asserted there
    assert got["three waves"][0] >= 6
