"""World data with a building set per env (rvo3d_amd/worlds.py): World.env_buildings / select, synthetic_world's
per-env generator, stack_worlds.  Host only."""
import numpy as np
import pytest

from rvo3d_amd import worlds
from rvo3d_amd.worlds import World, stack_worlds, synthetic_world

MAP = (40.0, 30.0, 10.0)


def _draw(rng, nb):
    """synthetic_world's docstring, restated: x,y ~U(2, L-2), h ~U(3, H), r ~U(0.5, 1.5), each a vector of nb drawn in
    that order, rounded to 2 decimals."""
    L, Wd, H = MAP
    return np.round(np.stack([rng.uniform(2, L - 2, nb), rng.uniform(2, Wd - 2, nb), rng.uniform(3, H, nb),
                              rng.uniform(0.5, 1.5, nb)], axis=1), 2)


def test_default_buildings_are_the_shared_philox_draw():
    w = synthetic_world(3, 4, MAP, nb=6, seed=77)
    assert w.buildings.shape == (6, 4) and w.building_counts is None and not w.per_env_buildings
    assert np.array_equal(w.buildings, _draw(np.random.Generator(np.random.Philox(key=78)), 6))
    w0 = synthetic_world(3, 4, MAP, seed=77)
    assert w0.buildings.shape == (0, 4)
    # the routes do not depend on the buildings' form
    wp = synthetic_world(3, 4, MAP, nb=6, seed=77, per_env_buildings=True)
    assert np.array_equal(w.waypoints, wp.waypoints) and np.array_equal(w.n_points, wp.n_points)


def test_per_env_sets_come_from_the_envs_own_stream_and_do_not_depend_on_E():
    w5 = synthetic_world(5, 4, MAP, nb=6, seed=77, per_env_buildings=True)
    w3 = synthetic_world(3, 4, MAP, nb=6, seed=77, per_env_buildings=True)
    assert w5.buildings.shape == (5, 6, 4) and w3.buildings.shape == (3, 6, 4) and w5.per_env_buildings
    assert w5.building_counts is None
    assert np.array_equal(w5.buildings[:3], w3.buildings)
    for e in range(5):
        rng = np.random.Generator(np.random.Philox(key=78, counter=[0, 0, 0, e]))
        assert np.array_equal(w5.buildings[e], _draw(rng, 6))
        assert np.array_equal(w5.env_buildings(e), w5.buildings[e])
    assert len({w5.buildings[e].tobytes() for e in range(5)}) == 5  # five different cities


def test_env_buildings_in_either_form():
    shared = synthetic_world(3, 4, MAP, nb=5, seed=3)
    for e in range(3):
        assert np.array_equal(shared.env_buildings(e), shared.buildings)
    b = np.arange(3 * 4 * 4, dtype=np.float64).reshape(3, 4, 4)
    w = World(shared.waypoints, shared.n_points, shared.map_size, b, np.array([0, 4, 2], np.int32))
    assert w.env_buildings(0).shape == (0, 4)
    assert np.array_equal(w.env_buildings(1), b[1]) and np.array_equal(w.env_buildings(2), b[2, :2])
    # positional construction with four fields, as everywhere else: no counts
    w4 = World(shared.waypoints, shared.n_points, shared.map_size, b)
    assert w4.building_counts is None and np.array_equal(w4.env_buildings(2), b[2])


def test_select_slices_routes_counts_and_per_env_buildings():
    base = synthetic_world(4, 3, MAP, n_points=3, nb=5, seed=9, per_env_buildings=True)
    w = World(base.waypoints, base.n_points, base.map_size, base.buildings, np.array([5, 0, 3, 1], np.int32))
    s = w.select([2, 0])
    assert s.shape == (2, 3, 3)
    assert np.array_equal(s.waypoints, w.waypoints[[2, 0]]) and np.array_equal(s.n_points, w.n_points[[2, 0]])
    assert np.array_equal(s.buildings, w.buildings[[2, 0]]) and np.array_equal(s.building_counts, [3, 5])
    assert np.array_equal(s.env_buildings(0), w.env_buildings(2)) and np.array_equal(s.env_buildings(1), w.env_buildings(0))
    assert np.array_equal(s.map_size, w.map_size)
    sl = w.select(slice(1, 3))
    assert sl.shape[0] == 2 and np.array_equal(sl.building_counts, [0, 3])
    m = w.select(np.array([True, False, False, True]))
    assert m.shape[0] == 2 and np.array_equal(m.env_buildings(1), w.env_buildings(3))
    # a shared list stays shared
    sh = synthetic_world(4, 3, MAP, nb=5, seed=9)
    ss = sh.select([3, 1])
    assert ss.buildings.shape == (5, 4) and np.array_equal(ss.buildings, sh.buildings) and ss.building_counts is None
    assert np.array_equal(ss.waypoints, sh.waypoints[[3, 1]])


def test_stack_worlds_keeps_equal_lists_shared():
    a = synthetic_world(2, 3, MAP, nb=4, seed=5)
    b = synthetic_world(3, 3, MAP, nb=4, seed=5)  # the same key: the same shared list
    s = stack_worlds([a, b])
    assert s.shape == (5, 3, 2) and s.buildings.shape == (4, 4) and s.building_counts is None
    assert np.array_equal(s.buildings, a.buildings)
    assert np.array_equal(s.waypoints, np.concatenate([a.waypoints, b.waypoints]))
    assert s.n_points.dtype == np.int32 and np.array_equal(s.n_points, np.concatenate([a.n_points, b.n_points]))
    # worlds without buildings stay a world without buildings
    e = stack_worlds([synthetic_world(1, 3, MAP, seed=1), synthetic_world(2, 3, MAP, seed=2)])
    assert e.buildings.shape == (0, 4) and e.building_counts is None


def test_stack_worlds_makes_differing_lists_per_env_with_counts_and_pads_routes():
    a = synthetic_world(2, 3, MAP, n_points=2, nb=4, seed=5)
    b = synthetic_world(1, 3, MAP, n_points=4, nb=6, seed=6)
    c = synthetic_world(2, 3, MAP, n_points=3, seed=7)  # no buildings
    s = stack_worlds([a, b, c])
    assert s.shape == (5, 3, 4) and s.buildings.shape == (5, 6, 4)
    assert np.array_equal(s.building_counts, [4, 4, 6, 0, 0]) and s.building_counts.dtype == np.int32
    for e, (w, we) in enumerate([(a, 0), (a, 1), (b, 0), (c, 0), (c, 1)]):
        assert np.array_equal(s.env_buildings(e), w.env_buildings(we))
        p = w.shape[2]
        assert np.array_equal(s.waypoints[e, :, :p], w.waypoints[we])
        # shorter routes: padded with the destination, as world_from_dict pads
        assert np.array_equal(s.waypoints[e, :, p:], np.repeat(w.waypoints[we][:, -1:], 4 - p, axis=1))
        assert np.array_equal(s.n_points[e], w.n_points[we])
    # equal lengths, different lists: per env, no counts needed
    d = stack_worlds([synthetic_world(1, 3, MAP, nb=4, seed=5), synthetic_world(1, 3, MAP, nb=4, seed=8)])
    assert d.buildings.shape == (2, 4, 4) and d.building_counts is None
    # a per-env world stacks env by env
    p = synthetic_world(2, 3, MAP, nb=4, seed=5, per_env_buildings=True)
    q = stack_worlds([p, a])
    assert q.buildings.shape == (4, 4, 4) and np.array_equal(q.env_buildings(1), p.buildings[1])
    assert np.array_equal(q.env_buildings(3), a.buildings)


def test_stack_worlds_pads_with_the_destination_of_short_routes():
    # a drone whose route is shorter than its world's P: the padding repeats waypoint n_points - 1
    a = synthetic_world(1, 2, MAP, n_points=3, seed=5)
    a.n_points[0, 1] = 2
    a.waypoints[0, 1, 2] = a.waypoints[0, 1, 1]
    b = synthetic_world(1, 2, MAP, n_points=5, seed=6)
    s = stack_worlds([a, b])
    assert np.array_equal(s.waypoints[0, 1, 2:], np.repeat(a.waypoints[0, 1, 1:2], 3, axis=0))
    assert np.array_equal(s.waypoints[0, 0, 3:], np.repeat(a.waypoints[0, 0, 2:3], 2, axis=0))


def test_stack_worlds_refuses_mismatched_drone_counts_and_maps():
    a = synthetic_world(2, 3, MAP, seed=5)
    with pytest.raises(ValueError):
        stack_worlds([a, synthetic_world(2, 4, MAP, seed=5)])
    with pytest.raises(ValueError):
        stack_worlds([a, synthetic_world(2, 3, (40.0, 30.0, 12.0), seed=5)])
    with pytest.raises(ValueError):
        stack_worlds([])
    assert worlds.stack_worlds is stack_worlds
