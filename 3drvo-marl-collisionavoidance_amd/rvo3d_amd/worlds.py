"""World data: the reference's `data_1.json` format (env_base.py:26-47) and the
synthetic generator of SURVEY.md section 8(d) used by bench.py and the tests."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field

import numpy as np


@dataclass
class World:
    """Routes for E envs x N drones plus buildings: one list shared by all envs, or a set per env."""
    waypoints: np.ndarray          # [E, N, P, 3] float64 (padded with the destination)
    n_points: np.ndarray           # [E, N] int32
    map_size: np.ndarray           # [3]
    # [nb, 4] x,y,h,r shared by every env, or [E, nb_max, 4]: env e's own set
    buildings: np.ndarray = field(default_factory=lambda: np.zeros((0, 4)))
    # per-env sets only: [E] int32, env e's set is buildings[e, :building_counts[e]] (None: all nb_max)
    building_counts: np.ndarray | None = None
    # fleets of different sizes: [E] int32, env e has the drones 0 .. drone_counts[e]-1 of its N rows, the rows beyond
    # are ghosts (BatchedDroneEnv.set_drone_counts); None: every env has N drones
    drone_counts: np.ndarray | None = None

    @property
    def shape(self):
        return self.waypoints.shape[:3]

    def env_drones(self, e: int) -> int:
        """The drones env e has."""
        return int(self.shape[1] if self.drone_counts is None else self.drone_counts[e])

    def with_drone_counts(self, counts) -> "World":
        """The same world with env e cut down to its first counts[e] drones (each 1..N; None: all N again)."""
        c = None
        if counts is not None:
            c = np.array(counts, dtype=np.int32)
            if c.shape != (self.shape[0],) or np.any(c < 1) or np.any(c > self.shape[1]):
                raise ValueError("with_drone_counts: counts must be [E] with entries in 1..N")
        return World(self.waypoints, self.n_points, self.map_size, self.buildings, self.building_counts, c)

    @property
    def per_env_buildings(self) -> bool:
        return np.ndim(self.buildings) == 3

    def env_buildings(self, e: int) -> np.ndarray:
        """Env e's building list [n, 4], whether the world shares one list or holds a set per env."""
        if not self.per_env_buildings:
            return self.buildings
        n = self.buildings.shape[1] if self.building_counts is None else int(self.building_counts[e])
        return self.buildings[e, :n]

    def with_max_points(self, P: int) -> "World":
        """The same world with the waypoint rows padded with each destination up to P rows: room for the detours a
        CityRoutePlanner inserts.  P below the rows in use is a ValueError."""
        wp = np.asarray(self.waypoints, dtype=np.float64)
        E, N, p = wp.shape[:3]
        if P < int(np.max(self.n_points, initial=2)):
            raise ValueError("with_max_points: P is below the longest route")
        last = np.take_along_axis(wp, (np.asarray(self.n_points).astype(np.int64) - 1)[:, :, None, None], axis=2)
        out = np.broadcast_to(last, (E, N, P, 3)).copy()
        k = min(p, P)
        used = np.arange(k)[None, None, :, None] < np.asarray(self.n_points)[:, :, None, None]
        out[:, :, :k] = np.where(used, wp[:, :, :k], out[:, :, :k])
        return World(out, np.array(self.n_points, dtype=np.int32), self.map_size, self.buildings, self.building_counts,
                     self.drone_counts)

    def select(self, envs) -> "World":
        """The world of the listed envs (indices, a slice or a mask over E); a shared list stays shared."""
        per = self.per_env_buildings
        cnt = self.building_counts[envs] if per and self.building_counts is not None else None
        return World(self.waypoints[envs], self.n_points[envs], self.map_size,
                     self.buildings[envs] if per else self.buildings, cnt,
                     None if self.drone_counts is None else np.asarray(self.drone_counts)[envs])


def world_from_dict(d: dict, num_envs: int = 1) -> World:
    """`data_1.json` keys: drone_num, map_size, waypoints_list, n_points_list,
    building_list (env_base.py:35-39).  The one scenario is replicated E times."""
    wl = d["waypoints_list"]
    N = int(d.get("drone_num", len(wl)))
    P = max(len(w) for w in wl)
    wp = np.zeros((N, P, 3))
    for i, w in enumerate(wl[:N]):
        w = np.asarray(w, dtype=np.float64)
        wp[i, :len(w)] = w
        wp[i, len(w):] = w[-1]
    npts = np.asarray(d["n_points_list"][:N], dtype=np.int32)
    bld = np.asarray(d.get("building_list", []), dtype=np.float64).reshape(-1, 4)
    return World(np.repeat(wp[None], num_envs, 0).copy(), np.repeat(npts[None], num_envs, 0).copy(),
                 np.asarray(d["map_size"], dtype=np.float64), bld)


def load_world_dir(base_dir: str, num_envs: int = 1) -> World:
    """env_base.load_data (env_base.py:26-47).  E3d.npy / E3d_safe.npy are
    optional: the reference loads them but never uses them numerically."""
    with open(os.path.join(base_dir, "data_1.json")) as f:
        return world_from_dict(json.load(f), num_envs)


def _draw_buildings(brng, nb: int, map_size) -> np.ndarray:
    L, Wd, H = map_size
    return np.round(np.stack([brng.uniform(2, L - 2, nb), brng.uniform(2, Wd - 2, nb),
                              brng.uniform(3, H, nb), brng.uniform(0.5, 1.5, nb)], axis=1), 2)


def synthetic_world(E: int, N: int, map_size, n_points: int = 2, nb: int = 0, seed: int = 1234,
                    min_sep: float = 1.0, per_env_buildings: bool = False) -> World:
    """per env e, rng = Philox(seed, stream e); starts/ends
    ~U([1, L-1]^2 x [1, H-1]) rounded to 2 decimals, starts at least min_sep
    apart; buildings [x,y ~U(2, L-2), h ~U(3, H), r ~U(0.5, 1.5)] rounded to 2 decimals: one list
    from Philox(seed + 1) shared by every env, or - per_env_buildings - env e's own nb buildings
    from Philox(seed + 1, stream e) (env e's set does not depend on E)."""
    L, Wd, H = map_size
    lo = np.array([1.0, 1.0, 1.0])
    hi = np.array([L - 1.0, Wd - 1.0, H - 1.0])
    wp = np.empty((E, N, n_points, 3))
    for e in range(E):
        rng = np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, 0, e]))
        pts = np.round(rng.uniform(lo, hi, (N, n_points, 3)), 2)
        starts = pts[:, 0]
        for i in range(1, N):  # rejection: keep starts min_sep apart
            tries = 0
            while tries < 200 and np.min(np.linalg.norm(starts[:i] - starts[i], axis=1)) < min_sep:
                starts[i] = np.round(rng.uniform(lo, hi), 2)
                tries += 1
        wp[e] = pts
    if per_env_buildings:
        bld = np.stack([_draw_buildings(np.random.Generator(np.random.Philox(key=seed + 1, counter=[0, 0, 0, e])),
                                        nb, map_size) for e in range(E)])
    else:
        brng = np.random.Generator(np.random.Philox(key=seed + 1))
        bld = _draw_buildings(brng, nb, map_size) if nb else np.zeros((0, 4))
    return World(wp, np.full((E, N), n_points, np.int32), np.asarray(map_size, dtype=np.float64), bld)


def stack_worlds(worlds, pad_drones: bool = False) -> World:
    """One batch of several worlds, concatenated along E: equal map sizes (ValueError otherwise), shorter routes padded
    with the destination.  Worlds of different drone counts are a ValueError too unless pad_drones: then every env is
    padded to the largest count with copies of its drone 0 route (n_points 2) and drone_counts [E] says how many
    drones each env has (None when they all have the same) - the padding rows are ghosts, never stepped.  The buildings
    stay one shared list when every world brings the same one; otherwise each env gets the list of the world it came
    from (building_counts where the lengths differ)."""
    worlds = list(worlds)
    if not worlds:
        raise ValueError("stack_worlds needs at least one world")
    N, m = max(w.shape[1] for w in worlds), np.asarray(worlds[0].map_size, dtype=np.float64)
    for w in worlds:
        if w.shape[1] != N and not pad_drones:
            raise ValueError("stack_worlds: the worlds have different drone counts (pad_drones=True pads them)")
        if not np.array_equal(np.asarray(w.map_size, dtype=np.float64), m):
            raise ValueError("stack_worlds: the worlds have different map sizes")
    P = max(w.shape[2] for w in worlds)
    wps, nps = [], []
    for w in worlds:
        wp = np.asarray(w.waypoints, dtype=np.float64)
        npt = np.asarray(w.n_points, dtype=np.int32)
        E, n, p = wp.shape[:3]
        if p < P:  # pad with each drone's destination, wp[e, i, n_points - 1]
            last = np.take_along_axis(wp, (npt.astype(np.int64) - 1)[:, :, None, None], axis=2)
            wp = np.concatenate([wp, np.broadcast_to(last, (E, n, P - p, 3))], axis=2)
        if n < N:  # ghost rows: the env's drone 0 route, cut to its first leg
            ghost = wp[:, :1].copy()
            ghost[:, :, 2:] = ghost[:, :, 1:2]
            wp = np.concatenate([wp, np.broadcast_to(ghost, (E, N - n, P, 3))], axis=1)
            npt = np.concatenate([npt, np.full((E, N - n), 2, np.int32)], axis=1)
        wps.append(wp)
        nps.append(npt)
    wp = np.concatenate(wps, 0)
    npts = np.concatenate(nps, 0)
    dcnt = np.concatenate([np.asarray([w.env_drones(e) for e in range(w.shape[0])], dtype=np.int32) for w in worlds])
    dcnt = None if np.all(dcnt == N) else dcnt
    lists = [np.asarray(w.env_buildings(e), dtype=np.float64).reshape(-1, 4) for w in worlds for e in range(w.shape[0])]
    if all(l.shape == lists[0].shape and np.array_equal(l, lists[0]) for l in lists):
        return World(wp, npts, m, lists[0].copy(), None, dcnt)
    nb_max = max(len(l) for l in lists)
    bld = np.zeros((len(lists), nb_max, 4))
    for e, l in enumerate(lists):
        bld[e, :len(l)] = l
    cnt = np.asarray([len(l) for l in lists], dtype=np.int32)
    return World(wp, npts, m, bld, None if np.all(cnt == nb_max) else cnt, dcnt)


def crossing_world(E: int, N: int, map_size, radius: float | None = None, alt_spread: float = 1.0,
                   angle_jitter: float = 0.05, radius_jitter: float = 0.5, min_sep: float = 1.0,
                   seed: int = 1234) -> World:
    """The classical RVO swap scene: per env, N starts on a horizontal ring around the map's centre c (angles evenly
    spaced with a random rotation per env and +-angle_jitter rad per drone, radius +-radius_jitter, altitude
    c_z +-alt_spread), each destination antipodal through the centre (2 c - start), rounded to 2 decimals; starts at
    least min_sep apart (a start that is too close is redrawn).  Every drone flies at the centre: the scene puts
    drones on collision course by construction (velocity-obstacle rows in the observations).  radius: default
    0.4 min(L, W).  rng = Philox(seed, stream e) per env, as synthetic_world."""
    L, Wd, H = (float(x) for x in map_size)
    c = np.array([L / 2, Wd / 2, H / 2])
    R = 0.4 * min(L, Wd) if radius is None else float(radius)
    if R + radius_jitter > min(L, Wd) / 2 - 1.0 or alt_spread > H / 2 - 1.0:
        raise ValueError("the ring does not fit inside the map (1 m margin)")
    wp = np.empty((E, N, 2, 3))

    def draw(rng, i, rot):
        a = rot + 2 * np.pi * i / N + rng.uniform(-angle_jitter, angle_jitter)
        rr = R + rng.uniform(-radius_jitter, radius_jitter)
        return np.round(c + np.array([rr * np.cos(a), rr * np.sin(a), rng.uniform(-alt_spread, alt_spread)]), 2)

    for e in range(E):
        rng = np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, 0, e]))
        rot = rng.uniform(0, 2 * np.pi)
        starts = np.empty((N, 3))
        for i in range(N):
            starts[i] = draw(rng, i, rot)
            tries = 0
            while i and tries < 200 and np.min(np.linalg.norm(starts[:i] - starts[i], axis=1)) < min_sep:
                starts[i] = draw(rng, i, rot)
                tries += 1
            if i and np.min(np.linalg.norm(starts[:i] - starts[i], axis=1)) < min_sep:
                raise ValueError(f"cannot place {N} starts {min_sep} m apart on a ring of radius {R}")
        wp[e, :, 0] = starts
        wp[e, :, 1] = np.round(2 * c - starts, 2)
    return World(wp, np.full((E, N), 2, np.int32), np.asarray(map_size, dtype=np.float64), np.zeros((0, 4)))


def synthetic_actions(E: int, N: int, step: int, seed: int = 1234) -> np.ndarray:
    """round(U(-1,1)^3 * [1, 0.3, 0.15], 2) from Philox(seed, step)."""
    rng = np.random.Generator(np.random.Philox(key=seed + 7, counter=[0, 0, 0, step]))
    return np.round(rng.uniform(-1, 1, (E, N, 3)) * np.array([1.0, 0.3, 0.15]), 2)
