"""Shared by tests/test_city_routes_host.py and tests/test_gpu_city_routes.py: the reference case of the city re-draw and
the dense check of a route against the env's own collision predicate.  Not a test module."""
import functools

import numpy as np

from rvo3d_amd import CityRoutePlanner, RouteSampler, synthetic_world

MAP = (40, 40, 10)
E, N, DRAW = 8, 70, 1


def planner(**kw):
    """clear_xy = clear_z = 0.5, pad = 0.25 over RouteSampler(min_sep 1, min_len 10, seed 7)."""
    return CityRoutePlanner(RouteSampler(MAP, min_sep=1.0, min_len=10.0, seed=7), **kw)


@functools.lru_cache(maxsize=None)
def city_world(envs=E, nb=12):
    return synthetic_world(envs, N, MAP, nb=nb, per_env_buildings=True, seed=5)


@functools.lru_cache(maxsize=None)
def reference(P):
    """The numpy re-draw of the reference case with P rows: (sampled waypoints, unplaced, planned waypoints, n_points,
    blocked, blocked_mask).  Computed once per P; nobody writes into it."""
    w, pl = city_world(), planner()
    wp, _, unp = pl.sample_numpy(E, N, P, DRAW, w.buildings)
    out = pl.plan_numpy(wp, w.buildings)
    for a in (wp, unp) + out:
        a.setflags(write=False)
    return (wp, unp) + out


def dense_hits(route, bld, step=0.01):
    """Does the polyline `route` [n, 3] touch a building of bld [nb, 4]?  Every leg is sampled at <= step and each
    sample is put to the env's predicate for a drone of radius 0.2: hypot(dx, dy) <= r + 0.2 and z <= h
    (rvo_inter.py:198-209).  Independent of the planner's own test."""
    for a, b in zip(route[:-1], route[1:]):
        n = int(np.ceil(np.linalg.norm(b - a) / step)) + 1
        p = a + np.linspace(0.0, 1.0, n)[:, None] * (b - a)
        near = np.hypot(p[:, None, 0] - bld[None, :, 0], p[:, None, 1] - bld[None, :, 1]) <= bld[None, :, 3] + 0.2
        if np.any(near & (p[:, None, 2] <= bld[None, :, 2])):
            return True
    return False
