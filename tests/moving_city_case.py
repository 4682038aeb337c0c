"""Shared by tests/test_moving_city_host.py, tests/test_gpu_moving_city.py and the second-pass case of
tests/test_gpu_rvo_city.py: the inputs of the moving-city tests and the CPU flights that count their non-vacuity figures.
No GPU needed; not a test module.

Everything is put together from what the suite already trusts: the building sets, patrols, actions and the numpy
trajectory of tests/test_gpu_building_motion.py, building_motion_ref.move, rvo_city_ref, safety_numpy, the numpy
restatements inside CityRoutePlanner, and the CPU oracle (one OracleEnv per env and step with that step's list, every env
flown alone at its drone count)."""
import functools
import types

import numpy as np

import oracle as orc
from rvo3d_amd import CityRoutePlanner, RouteSampler, World, synthetic_actions
from rvo3d_amd.safety import safety_numpy
import building_motion_ref as mref
import building_rows_moving_ref as ref8
import rvo_city_ref as ref
from test_gpu_building_motion import MAP, RADIUS, T, inputs, trajectory

# ---- the CPU's figures (the tables in the docstring of tests/test_gpu_moving_city.py; tests/test_moving_city_host.py
# recounts them) and the floors made from them: at most half, since glibc's and ocml's asin / acos may move a drone on a
# knife edge

TWIN_FIGURES = {(8, 21): (57, 197, 1965), (64, 6): (98, 333, 3574), (100, 3): (103, 288, 2810)}
REDRAW_STEPS = {(8, 21): (3, 6), (64, 6): (3, 6)}
REDRAW_CHANGES = {(8, 21): ((5, 11, 1), (6, 16, 5)), (64, 6): ((2, 13, 1), (2, 16, 5))}
REDRAW_FIGURES = {(8, 21, "plain"): ((43, 54), (31, 40)), (8, 21, "counted"): ((28, 33), (20, 24)),
                  (64, 6, "plain"): ((56, 121), (35, 61)), (64, 6, "counted"): ((45, 48), (21, 46))}
CITY_FLIPS = (5, 3, 0, 4)
CITY_FIGURES = dict(tier1=1827, tier2=17, tier3=112, moving_only=1369, arrival_gated=1107, records=6)
PASS_FIGURES = dict(tier3=137, distinct=36, distinct_64=21, from_192=2, first_tile_differs=2, mixed_envs=1)
TABLE_FIGURES = {"the wave seam, two tiles": (119, 16), "three waves": (12, 0)}


def floor(figure):
    """The non-vacuity floor for a figure the CPU counted."""
    return max(figure // 2, 1)


# ---- 1. counted handles in a moving city ---------------------------------------------------------------------------------------

SHAPES = [(8, 21), (64, 6), (100, 3)]
# the counts a handle starts with (cycled over the envs; env e has building set e % 3) and what step CHANGE_AT sets; at
# RESTORE_AT the counts are taken off (None).  Every shape has a 1, an N and a count that is no multiple of any packed
# row width (3, 5, 7; 33, 63; 33); 100 x 3 has counts <= 36: the second wave of those envs is ghosts alone.
CHANGE_AT, RESTORE_AT = 8, 16
START = {(8, 21): (8, 1, 3, 5, 2, 8, 7), (64, 6): (64, 33, 48, 1, 63, 2), (100, 3): (1, 100, 33)}
CHANGED = {(64, 6): (64, 48, 20, 30, 63, 2), (100, 3): (65, 20, 33)}


def start_counts(N, E):
    cyc = START[(N, E)]
    return np.array([cyc[e % len(cyc)] for e in range(E)], dtype=np.int32)


def changed_counts(N, E):
    """The counts of step CHANGE_AT: some envs go up, some down, some stay - in 8 x 21 every fourth env takes its
    neighbour's count, which reaches envs of all three building sets."""
    c1 = start_counts(N, E)
    if (N, E) in CHANGED:
        c2 = np.array(CHANGED[(N, E)], dtype=np.int32)
    else:
        c2 = c1.copy()
        c2[0::4] = np.roll(c1, 1)[0::4]
    assert (c2 > c1).any() and (c2 < c1).any() and (c2 == c1).any()
    return c2


def counts_at(N, E, t, schedule=True):
    """The counts in force during step t (None: every env has N drones)."""
    if not schedule or t < CHANGE_AT:
        return start_counts(N, E)
    return changed_counts(N, E) if t < RESTORE_AT else None


def actions(N, E, t, counts=None):
    """synthetic_actions(E, N, t, 1234), NaN in the ghosts' rows."""
    a = synthetic_actions(E, N, t, 1234)
    if counts is not None:
        a[np.arange(N)[None, :] >= np.asarray(counts)[:, None]] = np.nan
    return a


@functools.lru_cache(maxsize=None)
def cpu_flight(N, E, moving, schedule=True):
    """The counted twin's run on the CPU, plain steps + reset of the drones that are done or have finished: every env
    alone at its count in an OracleEnv with that step's list (the numpy trajectory; moving False: the sets stand still),
    the envs whose count changes start again from their reset state.  Returns done [T, E, N] bool and bclear [T, E, N]
    (safety_numpy on the positions behind the step; ghost rows False / +inf)."""
    world, _, _ = inputs(N, E)
    pos, _ = trajectory(N, E)
    state = [None] * E
    prev = None
    done_all, bclear_all = np.zeros((T, E, N), bool), np.full((T, E, N), np.inf)
    for t in range(T):
        cnt = counts_at(N, E, t, schedule)
        cnt = np.full(E, N, np.int32) if cnt is None else cnt
        bld = pos[t + 1] if moving else pos[0]
        after = np.zeros((E, N, 3))
        for e in range(E):
            c, nb = int(cnt[e]), int(world.building_counts[e])
            if prev is not None and prev[e] != c:
                state[e] = None
            env = orc.OracleEnv(world.waypoints[e:e + 1, :c], world.n_points[e:e + 1, :c], world.map_size, bld[e, :nb],
                                radius=np.full((1, c), RADIUS))
            env.reset()
            if state[e] is not None:
                env.set_state(**state[e])
            _, _, _, done, _, fin = env.step(actions(N, E, t)[e:e + 1, :c])
            after[e, :c] = env.get_state()["pos"][0]
            done_all[t, e, :c] = done[0] != 0
            env.reset_drones((done != 0) | (fin != 0))
            state[e] = env.get_state()
        bclear_all[t] = safety_numpy(after, RADIUS, world.map_size, 0.5, counts=cnt, buildings=bld,
                                     building_counts=world.building_counts)[1]
        prev = [int(x) for x in cnt]
    return done_all, bclear_all


def twin_figures(N, E):
    """(done flags of live drones that differ between the moving and the standing city inside the envs of set B, of set C,
    bclear entries that differ) over the T steps."""
    dm, bm = cpu_flight(N, E, True)
    ds, bs = cpu_flight(N, E, False)
    diff = dm != ds
    return int(diff[:, 1::3].sum()), int(diff[:, 2::3].sum()), int((bm != bs).sum())


# ---- 2. re-draws round the buildings where they are now ---------------------------------------------------------------------

REDRAW_SHAPES = [(8, 21), (64, 6)]
P_REDRAW = 6          # rows per route: room for four detour points
DRAWS = (1, 2)        # the draw numbers of the two re-draws


def planner():
    """test_gpu_city_routes.py's constructor values (min_sep 1, min_len 10, seed 7; clear_xy = clear_z = 0.5, pad 0.25)
    on the map of the moving sets."""
    return CityRoutePlanner(RouteSampler(MAP, min_sep=1.0, min_len=10.0, seed=7))


def redraw_world(N, E):
    return inputs(N, E)[0].with_max_points(P_REDRAW)


def _cells(p, e, n):
    return mref.cell_of(p[e, :n, 0], p[e, :n, 1], 3, 3)


def changes_between(N, E, t0, t1):
    """(buildings of set B, of set C whose cell at t1 is not their cell at t0, records whose leg flipped in a step of
    (t0, t1]) of the reference trajectory."""
    world, _, _ = inputs(N, E)
    pos, legs = trajectory(N, E)
    n = world.building_counts
    moved = [int((_cells(pos[t1], s, int(n[s])) != _cells(pos[t0], s, int(n[s]))).sum()) for s in (1, 2)]
    flips = sum(int((legs[t + 1][:3] != legs[t][:3]).sum()) for t in range(t0, t1))
    return moved[0], moved[1], flips


@functools.lru_cache(maxsize=None)
def redraw_steps(N, E):
    """t1 < t2: the first steps (from 3 on, at least 3 apart) before each of which - since the start for t1, since t1 for
    t2 - a building of B and one of C has changed its cell and a record has flipped leg."""
    out, t0 = [], 0
    for _ in range(2):
        t = next(t for t in range(t0 + 3, T - 3) if min(changes_between(N, E, t0, t)) >= 1)
        out.append(t)
        t0 = t
    return tuple(out)


def redraw_mask(E):
    """The env_mask of the second re-draw: the last env of every set stays out, and with more than six envs the first."""
    m = np.ones(E, bool)
    m[-3:] = False
    if E > 6:
        m[:3] = False
    return m


@functools.lru_cache(maxsize=None)
def restated_redraw(N, E, t, draw):
    """sample_numpy + plan_numpy round the buildings of trajectory()[t]: (waypoints, n_points, unplaced, blocked)."""
    world, _, _ = inputs(N, E)
    pos, _ = trajectory(N, E)
    pl = planner()
    wp, _, unp = pl.sample_numpy(E, N, P_REDRAW, draw, pos[t], world.building_counts)
    wp, npts, blocked, _ = pl.plan_numpy(wp, pos[t], world.building_counts)
    for a in (wp, npts, unp, blocked):
        a.setflags(write=False)
    return wp, npts, unp, blocked


def redraw_figures(N, E, counts=None):
    """Per re-draw: (live drones of B envs, of C envs - at the second re-draw those inside its env_mask - whose route round
    the buildings of step t is not their route round the start positions)."""
    live = np.ones((E, N), bool) if counts is None else np.arange(N)[None, :] < np.asarray(counts)[:, None]
    out = []
    for k, (t, draw) in enumerate(zip(redraw_steps(N, E), DRAWS)):
        now, stale = restated_redraw(N, E, t, draw), restated_redraw(N, E, 0, draw)
        diff = ((now[0] != stale[0]).any(axis=(2, 3)) | (now[1] != stale[1])) & live
        if k:  # the second re-draw is masked
            diff &= redraw_mask(E)[:, None]
        out.append((int(diff[1::3].sum()), int(diff[2::3].sum())))
    return out


# ---- 3. the city controller and the evaluator along a flown trajectory -------------------------------------------------------

CITY_MAP = (20.0, 16.0, 8.0)
CITY_E, CITY_N, CITY_NB = 4, 65, 6
CITY_COUNTS = np.array([65, 64, 1, 33], dtype=np.int32)
CITY_BCOUNTS = np.array([6, 5, 0, 6], dtype=np.int32)
CITY_STEPS, CITY_EP_LEN, CITY_RADIUS = 12, 6, 0.4
CITY_SEED, CITY_CLEAR, CITY_SEP = 2025, 3, 0.3
CITY_KW = dict(clear_xy=0.25, clear_z=0.5)     # the other parameters are rvo_vel_city's defaults
CITY_FILLER = np.array([10.0, 8.0, 100.0, 30.0])


@functools.lru_cache(maxsize=None)
def city_scene():
    """E 4, N 65, counts (65, 64, 1, 33), nb_max 6, building counts (6, 5, 0, 6), map (20, 16, 8).  Routes: starts at
    least 0.7 apart, goals at least 6 m from them.  Record 0 of an env stands still, records 1 - 3 patrol a short
    segment (they arrive and flip several times within 12 steps), records 4 and 5 cruise over 9 - 13 m."""
    rng = np.random.default_rng(CITY_SEED)
    E, N, nb = CITY_E, CITY_N, CITY_NB
    bld = np.empty((E, nb, 4))
    bld[:] = CITY_FILLER
    ends, speed = np.zeros((E, nb, 2, 2)), np.full((E, nb), 9.0)
    for e in range(E):
        n = int(CITY_BCOUNTS[e])
        b = np.round(np.stack([rng.uniform(3, 17, n), rng.uniform(3, 13, n), rng.uniform(3, 10, n), rng.uniform(0.8, 1.5, n)],
                              axis=1), 2)
        bld[e, :n] = b
        ends[e, :n, 0] = ends[e, :n, 1] = b[:, :2]
        speed[e, :n] = 0.0
        for j in range(1, n):
            ang = rng.uniform(0, 2 * np.pi)
            length = rng.uniform(2.0, 3.6) if j <= 3 else rng.uniform(9.0, 13.0)
            ends[e, j, 1] = np.clip(b[j, :2] + length * np.array([np.cos(ang), np.sin(ang)]), 1.0, np.array(CITY_MAP[:2]) - 1.0)
            speed[e, j] = np.round(rng.uniform(0.7, 1.2), 2)
    # where the buildings are during the first CITY_CLEAR steps: the starts keep 0.75 m clear of them
    rec, leg, early = bld.copy(), np.ones((E, nb), np.uint8), [bld.copy()]
    rec[np.arange(nb)[None, :] >= CITY_BCOUNTS[:, None], 2] = -np.inf
    for _ in range(CITY_CLEAR):
        rec, leg = mref.move(rec, ends, speed, leg, 1.0)
        early.append(rec.copy())
    lo, hi = np.array([1.0, 1.0, 1.0]), np.array(CITY_MAP) - 1.0
    wp = np.zeros((E, N, 2, 3))
    for e in range(E):
        n = int(CITY_BCOUNTS[e])
        near = np.concatenate([p[e, :n] for p in early])
        starts = []
        while len(starts) < N:
            p = np.round(rng.uniform(lo, hi), 2)
            if (np.hypot(near[:, 0] - p[0], near[:, 1] - p[1]) < near[:, 3] + CITY_RADIUS + 0.75).any():
                continue
            if all(np.linalg.norm(p - q) >= 2 * CITY_RADIUS + CITY_SEP for q in starts):
                starts.append(p)
        for d, p in enumerate(starts):
            while True:
                g = np.round(rng.uniform(lo, hi), 2)
                if np.linalg.norm(g - p) >= 6.0:
                    break
            wp[e, d, 0], wp[e, d, 1] = p, g
    world = World(wp, np.full((E, N), 2, np.int32), np.array(CITY_MAP), bld, CITY_BCOUNTS.copy(), CITY_COUNTS.copy())
    return types.SimpleNamespace(world=world, ends=ends, speed=speed, bld0=bld)


@functools.lru_cache(maxsize=None)
def city_trajectory(steps=CITY_STEPS):
    """positions[t] [E, 6, 4] (fillers as the scene has them) and leg[t] after t reference moves."""
    sc = city_scene()
    live = np.arange(CITY_NB)[None, :] < CITY_BCOUNTS[:, None]
    rec = sc.bld0.copy()
    rec[~live, 2] = -np.inf
    leg = np.ones((CITY_E, CITY_NB), np.uint8)
    pos, legs = [sc.bld0.copy()], [leg]
    for _ in range(steps):
        rec, leg = mref.move(rec, sc.ends, sc.speed, leg, 1.0)
        p = rec.copy()
        p[~live] = CITY_FILLER
        pos.append(p); legs.append(leg)
    return pos, legs


def city_flips():
    """Records per env that arrive and flip leg at least once within the CITY_STEPS moves."""
    _, legs = city_trajectory()
    return (np.stack(legs)[1:] != np.stack(legs)[:-1]).any(0).sum(1)


def arrivals(pos, seen, e, leg):
    """Gated (drone, record) pairs of env e whose record is on the arrival branch of the velocity rule (the rest of the
    way over dt): pos [c, 3] the env's live drones, seen [n, 4] its live records, leg [nb_max]."""
    sc = city_scene()
    arr = [j for j in range(len(seen)) if ref8.velocity(seen[j], sc.ends[e, j], sc.speed[e, j], leg[j], 1.0)[2] == 1]
    return sum(1 for p in pos for j in arr if ref.gate(p, seen[j])[0])


def fold_episodes(bclear_min, ended):
    """Per env the list of its episodes' minima: bclear_min [steps, E] (the minimum over an env's drones behind every
    step), ended [steps, E] bool; folded as rvo3d_eval_account_safety folds (x < m ? x : m from +inf)."""
    steps, E = bclear_min.shape
    out, run = [[] for _ in range(E)], np.full(E, np.inf)
    for t in range(steps):
        run = np.where(bclear_min[t] < run, bclear_min[t], run)
        for e in np.flatnonzero(ended[t]):
            out[e].append(run[e])
            run[e] = np.inf
    return out


@functools.lru_cache(maxsize=None)
def cpu_city_flight(moving=True):
    """The evaluator's loop with the city controller on the CPU: rvo_city_ref's rules over ref.drone_side, the oracle's
    plain step with the list of that step, safety_numpy behind it; an env's episode ends when one of its drones is done,
    at CITY_EP_LEN steps or when all have finished, and the env starts again (the buildings do not).  moving False: the
    same evaluation with the motion left out.  Returns dict(tiers: Counter of tier per drone and step, moving_only:
    candidate bits blocked with the motion and free with every record standing, arrival_gated: gated (drone, record)
    pairs on the arrival branch of the velocity rule, episodes: per env the list of its episodes' minimum bclear,
    episodes_early: the same with every scan made against the buildings where they were before that step's move)."""
    import collections
    sc = city_scene()
    w = sc.world
    pos, legs = city_trajectory()
    E, N = CITY_E, CITY_N
    state, ep_len = [None] * E, np.zeros(E, np.int64)
    tiers, moving_only, arrival_gated = collections.Counter(), 0, 0
    bmin, ended = np.full((CITY_STEPS, E), np.inf), np.zeros((CITY_STEPS, E), bool)
    bmin_early = bmin.copy()
    still = lambda j: (0.0, 0.0, 0)
    scratch = collections.Counter()
    for t in range(CITY_STEPS):
        after = np.zeros((E, N, 3))
        for e in range(E):
            c, nb = int(CITY_COUNTS[e]), int(CITY_BCOUNTS[e])
            seen = (pos[t] if moving else pos[0])[e, :nb]          # what the controller sees
            hit = (pos[t + 1] if moving else pos[0])[e, :nb]       # what the step collides with
            env = orc.OracleEnv(w.waypoints[e:e + 1, :c], w.n_points[e:e + 1, :c], w.map_size, hit,
                                radius=np.full((1, c), CITY_RADIUS))
            env.reset()
            if state[e] is not None:
                env.set_state(**state[e])
            s, des = env.get_state(), env.des_vel()
            vel_of = still
            if moving:
                vel_of = lambda j, e=e, seen=seen: ref8.velocity(seen[j], sc.ends[e, j], sc.speed[e, j], legs[t][e, j], 1.0)
            a = np.zeros((1, c, 3))
            rad, prio = np.full(c, CITY_RADIUS), np.ones(c)
            for i in range(c):
                vals, cnt, live = ref.candidates(s["vel"][0, i])
                cone, tc_min = ref.drone_side(i, s["pos"][0], s["vel"][0], rad, prio, vals, cnt, live)
                blocked, n_gated, tb = ref.sweep(s["pos"][0, i], CITY_RADIUS, vals, cnt, live, seen, vel_of, tally=scratch,
                                                 **CITY_KW)
                tier, a[0, i] = ref.select(vals, cnt, live, cone, blocked, tb, tc_min, des[0, i], tally=scratch)
                tiers[tier] += 1
                if moving and n_gated:
                    b0, _, _ = ref.sweep(s["pos"][0, i], CITY_RADIUS, vals, cnt, live, seen, still, tally=scratch, **CITY_KW)
                    moving_only += bin(blocked & ~b0).count("1")
            if moving:
                arrival_gated += arrivals(s["pos"][0], seen, e, legs[t][e])
            _, _, _, done, _, fin = env.step(a)
            after[e, :c] = env.get_state()["pos"][0]
            ep_len[e] += 1
            ended[t, e] = bool(done.any()) or ep_len[e] == CITY_EP_LEN or bool(fin.all())
            state[e] = env.get_state()
            if ended[t, e]:
                state[e], ep_len[e] = None, 0
        hit = pos[t + 1] if moving else pos[0]
        bclear = safety_numpy(after, CITY_RADIUS, w.map_size, 0.5, counts=CITY_COUNTS, buildings=hit,
                              building_counts=CITY_BCOUNTS)[1]
        bmin[t] = bclear.min(axis=1)
        early = safety_numpy(after, CITY_RADIUS, w.map_size, 0.5, counts=CITY_COUNTS, buildings=pos[t] if moving else pos[0],
                             building_counts=CITY_BCOUNTS)[1]
        bmin_early[t] = early.min(axis=1)
    return dict(tiers=tiers, moving_only=moving_only, arrival_gated=arrival_gated, episodes=fold_episodes(bmin, ended),
                episodes_early=fold_episodes(bmin_early, ended))


def city_figures():
    """(drones and steps in tier 1, 2, 3, moving_only, arrival_gated, first-two-episode records whose minimum bclear is
    not that of the evaluation without the motion)."""
    m, s = cpu_city_flight(True), cpu_city_flight(False)
    differ = sum(int(a != b) for e in range(CITY_E) for a, b in zip(m["episodes"][e][:2], s["episodes"][e][:2]))
    differ += sum(abs(min(len(m["episodes"][e]), 2) - min(len(s["episodes"][e]), 2)) for e in range(CITY_E))
    return m["tiers"][1], m["tiers"][2], m["tiers"][3], m["moving_only"], m["arrival_gated"], differ


# ---- 4. the second pass of the city kernel -------------------------------------------------------------------------------------

PASS_MAP = (20.0, 16.0, 8.0)      # test_gpu_rvo_city.py's
PASS_MOVES = 3                    # ... and its MOVES
PASS_E, PASS_N, PASS_NB, PASS_TILE = 2, 130, 193, 192
PASS_COUNTS = (130, 100)
MAST = (0.1, 0.3)
PASS_KW = dict(vmax=(2.0, 2.0, 2.0), acceler=1.0, horizon=5.0, reach=10.0, below=1.0, clear_xy=0.25, clear_z=0.5)


@functools.lru_cache(maxsize=None)
def second_pass_scene():
    """A counted handle, E 2, N 130 (three waves: T = 192), counts (130, 100), nb_max 193 = T + 1, acceler 1 (64
    candidates).  Both envs are a forest of thin masts (r 0.3 .. 0.8) that no drone flies over, dense enough that many
    drones find every candidate blocked, at a different time each.  Env 0 has all 193 records; record 192 - alone in the
    second tile - is a disk of r 1.5 that crosses the forest at 2 m per step and is the first thing many candidates meet.
    Env 1 has 192 records (record 192 is a filler) of roofs below 5 m: its drones 0 .. 63 fly at 7.5 m, over every roof -
    nothing passes their gate, the first wave needs no second pass -, the others fly low among the masts."""
    rng = np.random.default_rng(4)
    E, N, nb = PASS_E, PASS_N, PASS_NB
    pos = rng.uniform(0.0, 1.0, (E, N, 3)) * np.array([PASS_MAP[0], PASS_MAP[1], 3.0]) + [0.0, 0.0, 0.5]
    pos[1, :64, 2] = 7.5
    ang, spd = rng.uniform(0, 2 * np.pi, (E, N)), rng.uniform(0.8, 2.0, (E, N))
    vel = np.stack([spd * np.cos(ang), spd * np.sin(ang), rng.uniform(-1, 1, (E, N))], axis=-1)
    rad = np.round(rng.uniform(0.1, 0.4, (E, N)), 3)
    wp = np.zeros((E, N, 2, 3))
    wp[:, :, 0], wp[:, :, 1] = [1.0, 1.0, 1.0], [15.0, 9.0, 5.0]
    bld0 = np.concatenate([rng.uniform(0, PASS_MAP[0], (E, nb, 1)), rng.uniform(0, PASS_MAP[1], (E, nb, 1)),
                           rng.uniform(20.0, 30.0, (E, nb, 1)), rng.uniform(MAST[0], MAST[1], (E, nb, 1))], axis=-1)
    bld0[1, :, 2] = rng.uniform(4.0, 5.0, nb)
    cnt = np.array([nb, nb - 1], dtype=np.int32)
    ends = np.zeros((E, nb, 2, 2))
    ends[:, :, 0] = bld0[..., :2]
    ends[:, :, 1] = bld0[..., :2] + rng.uniform(-6, 6, (E, nb, 2))
    speed = rng.uniform(0.3, 1.5, (E, nb))
    speed[:, ::3] = 0.0
    bld0[0, nb - 1] = [2.0, 8.0, 25.0, 1.5]
    ends[0, nb - 1], speed[0, nb - 1] = [[2.0, 8.0], [18.0, 8.0]], 2.0
    pos[0, 100], vel[0, 100] = [8.4, 8.3, 2.0], [1.2, 0.7, 0.0]      # inside record 192's disk after the moves
    pos[0, 101], vel[0, 101] = [11.5, 8.1, 2.0], [1.2, -0.7, 0.0]    # in its path, 3.5 m ahead
    dc = np.array(PASS_COUNTS, dtype=np.int32)
    world = World(wp, np.full((E, N), 2, np.int32), np.array(PASS_MAP), bld0, cnt, dc)
    return types.SimpleNamespace(E=E, N=N, pos=pos, vel=vel, rad=rad, drone_counts=dc, cnt=cnt, ends=ends, speed=speed,
                                 bld0=bld0, world=world)


@functools.lru_cache(maxsize=None)
def second_pass_now():
    """(buildings, leg) after PASS_MOVES reference moves: what the device holds when the kernel runs."""
    sc = second_pass_scene()
    live = np.arange(PASS_NB)[None, :] < sc.cnt[:, None]
    rec = sc.bld0.copy()
    rec[~live, 2] = -np.inf
    leg = np.ones((PASS_E, PASS_NB), np.uint8)
    for _ in range(PASS_MOVES):
        rec, leg = mref.move(rec, sc.ends, sc.speed, leg, 1.0)
    rec[~live] = sc.bld0[~live]
    return rec, leg


def second_pass_figures(sc, bld, leg, tier, live_mask, des, kw=PASS_KW):
    """From a restatement's tier and the live masks and des it was made from, over the tier-3 lanes: dict(tier3, distinct:
    lanes whose blocked candidates have at least two distinct tb, distinct_64: those with lane index >= 64, from_192: lanes
    whose winning candidate's least tb comes from record 192 - leaving the second tile out gives that candidate a later
    time or none -, first_tile_differs: lanes whose velocity is another one when tb is taken from the first tile alone,
    mixed_envs: envs with a wave without a tier-3 lane and a wave with one)."""
    import collections
    scratch = collections.Counter()
    out = dict(tier3=0, distinct=0, distinct_64=0, from_192=0, first_tile_differs=0, mixed_envs=0)
    par = {k: kw[k] for k in ("horizon", "reach", "below", "clear_xy", "clear_z")}
    for e in range(sc.E):
        n, c = int(sc.cnt[e]), int(sc.drone_counts[e])
        be = bld[e, :n]
        vel_of = lambda j, e=e, be=be: ref8.velocity(be[j], sc.ends[e, j], sc.speed[e, j], leg[e, j], 1.0)
        waves = [bool((tier[e, w0:min(w0 + 64, c)] == 3).any()) for w0 in range(0, c, 64)]
        out["mixed_envs"] += int(any(waves) and not all(waves))
        for d in np.flatnonzero(tier[e, :c] == 3):
            vals, cnt, _ = ref.candidates(sc.vel[e, d], kw["vmax"], kw["acceler"])
            lv = int(live_mask[e, d]) & (2 ** 64 - 1)
            blocked, _, tb = ref.sweep(sc.pos[e, d], sc.rad[e, d], vals, cnt, lv, be, vel_of, tally=scratch, **par)
            assert blocked == lv != 0
            _, tb1 = ref.sweep(sc.pos[e, d], sc.rad[e, d], vals, cnt, lv, be[:PASS_TILE], vel_of, tally=scratch, **par)[1:]
            tb1 = {k: tb1.get(k, ref.INF) for k in tb}
            _, v = ref.select(vals, cnt, lv, 0, blocked, tb, ref.INF, des[e, d], tally=scratch)
            _, v1 = ref.select(vals, cnt, lv, 0, blocked, tb1, ref.INF, des[e, d], tally=scratch)
            win = [k for k in tb if [vals[0][k // (cnt[1] * cnt[2])], vals[1][k // cnt[2] % cnt[1]], vals[2][k % cnt[2]]] == v]
            two = len(set(tb.values())) >= 2
            out["tier3"] += 1
            out["distinct"] += int(two)
            out["distinct_64"] += int(two and d >= 64)
            out["from_192"] += int(any(tb[k] < tb1[k] for k in win))
            out["first_tile_differs"] += int(v1 != v)
    return out


@functools.lru_cache(maxsize=None)
def second_pass_cpu():
    """second_pass_figures of the restatement on the CPU: rule 0's own live masks, des from the oracle.  (Tier 3 is "every
    live candidate blocked", whatever the drones' cones say, so the drone side is not needed to count it.)"""
    import collections
    sc = second_pass_scene()
    bld, leg = second_pass_now()
    scratch = collections.Counter()
    tier, live = np.zeros((sc.E, sc.N), np.int32), np.zeros((sc.E, sc.N), np.uint64)
    des = np.zeros((sc.E, sc.N, 3))
    par = {k: PASS_KW[k] for k in ("horizon", "reach", "below", "clear_xy", "clear_z")}
    for e in range(sc.E):
        n, c = int(sc.cnt[e]), int(sc.drone_counts[e])
        env = orc.OracleEnv(sc.world.waypoints[e:e + 1, :c], sc.world.n_points[e:e + 1, :c], sc.world.map_size, bld[e, :n],
                            radius=sc.rad[e:e + 1, :c])
        env.reset()
        env.set_state(pos=sc.pos[e:e + 1, :c], vel=sc.vel[e:e + 1, :c])
        des[e, :c] = env.des_vel()[0]
        vel_of = lambda j, e=e: ref8.velocity(bld[e, j], sc.ends[e, j], sc.speed[e, j], leg[e, j], 1.0)
        for d in range(c):
            vals, cnt, lv = ref.candidates(sc.vel[e, d], PASS_KW["vmax"], PASS_KW["acceler"])
            blocked, _, _ = ref.sweep(sc.pos[e, d], sc.rad[e, d], vals, cnt, lv, bld[e, :n], vel_of, tally=scratch, **par)
            live[e, d] = lv
            tier[e, d] = 3 if lv and blocked == lv else 1
    return second_pass_figures(sc, bld, leg, tier, live, des)


def distinct_tb_lanes(sc, bld, mot, tier, live_mask, kw):
    """Tier-3 lanes of a restatement whose blocked candidates have at least two distinct tb (the sweep again, on the live
    masks the restatement was made from).  sc: a scene of test_gpu_rvo_city.py, mot: (ends, speed, leg)."""
    import collections
    scratch = collections.Counter()
    par = {k: kw[k] for k in ("horizon", "reach", "below", "clear_xy", "clear_z")}
    n_two = 0
    for e, d in zip(*np.nonzero(tier == 3)):
        be = bld[e, :int(sc.cnt[e])] if bld.ndim == 3 else bld
        vel_of = (lambda j: (0.0, 0.0, 0)) if mot is None else (
            lambda j: ref8.velocity(be[j], mot[0][e, j], mot[1][e, j], mot[2][e, j], 1.0))
        vals, cnt, _ = ref.candidates(sc.vel[e, d], kw["vmax"], kw["acceler"])
        _, _, tb = ref.sweep(sc.pos[e, d], sc.rad[e, d], vals, cnt, int(live_mask[e, d]) & (2 ** 64 - 1), be, vel_of,
                             tally=scratch, **par)
        n_two += int(len(set(tb.values())) >= 2)
    return n_two


def table_figures():
    """The tier-3 figures of two CASES of test_gpu_rvo_city.py, counted on the CPU with the scene's positions after three
    reference moves: {case: (tier-3 lanes, of those with at least two distinct tb)}."""
    import collections
    import test_gpu_rvo_city as g
    scratch = collections.Counter()
    out = {}
    for E, N, nb_max, acceler, vmax, dc, what in g.CASES:
        if what not in ("the wave seam, two tiles", "three waves"):
            continue
        sc = g.scene(E, N, nb_max, dc)
        live = np.arange(nb_max)[None, :] < sc.cnt[:, None]
        rec, leg = sc.bld0.copy(), np.ones((E, nb_max), np.uint8)
        rec[~live, 2] = -np.inf
        for _ in range(g.MOVES):
            rec, leg = mref.move(rec, sc.ends, sc.speed, leg, g.DT)
        t3 = two = 0
        for e in range(E):
            n = int(sc.cnt[e])
            vel_of = lambda j, e=e: ref8.velocity(rec[e, j], sc.ends[e, j], sc.speed[e, j], leg[e, j], g.DT)
            for d in range(N):
                vals, cnt, lv = ref.candidates(sc.vel[e, d], vmax, acceler)
                blocked, _, tb = ref.sweep(sc.pos[e, d], sc.rad[e, d], vals, cnt, lv, rec[e, :n], vel_of, 5.0, 10.0, 1.0,
                                           0.25, 0.5, tally=scratch)
                if lv and blocked == lv:
                    t3 += 1
                    two += int(len(set(tb.values())) >= 2)
        out[what] = (t3, two)
    return out
