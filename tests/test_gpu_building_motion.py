"""Moving buildings (rvo3d_move_env_buildings; BatchedDroneEnv.attach_building_motion) on the GPU.

The yardstick is the host path, which test_gpu_env_buildings.py pins to the shared list and test_gpu_parity.py to the
reference: a handle M whose sets are moved on the device must behave bit for bit as a handle H that is given the same
positions - the numpy reference's (building_motion_ref.py) - through set_env_buildings before every step.  Further tests
make sure the comparison is not vacuous: buildings change their cell, set C's clustered cell goes between overflowing and
not, and the moving buildings change the done flags.

Inputs (the recipe of test_gpu_env_buildings.py, restated): map (24, 24, 8) - 3 x 3 cells of 8 m -,
synthetic_world(E, N, map, min_sep=0.8, seed=41), radius 0.2, synthetic_actions(E, N, t, 1234), 25 steps, nb_max 40.  Env e
gets set e % 3: A empty, B 10 buildings, C 40 buildings of which 20 start inside the cell [8, 16]^2.  Every building
patrols between its position and a second endpoint in another cell (the segment crosses x or y = 8 or 16) at a speed
~U(0.3, 1.5) per step; every seventh stands still (speed 0).

The same inputs on the CPU, before any GPU run - the numpy reference for the buildings, the CPU oracle for the drones (one
OracleEnv per env and step with that step's list and set_state, stepped without auto-reset, the drones that are done or
have finished reset after every step) - gave, over the 25 steps: buildings of B / of C that change their cell at least
once, steps in which C's centre cell overflows / does not, done flags of the moving run that differ from the run with
the same sets left static, inside the envs of B / of C:

    N x E     B movers  C movers  C overflows / not   B flags  C flags
    8 x 21           9        35            15 / 10       100      241
    64 x 6           9        35            15 / 10       119      708
    100 x 3          9        35            18 / 7        166      499

(The one building of B and the five of C that never change their cell are the ones that stand still.  C's cluster
patrols to the corners of the map, so that the centre cell empties and fills again.)
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from rvo3d_amd import (BatchedDroneEnv, BuildingMotion, BuildingObsEnv, World, _lib, synthetic_actions, synthetic_patrols,
                       synthetic_world)
import building_motion_ref as ref

pytestmark = pytest.mark.gpu

MAP = (24.0, 24.0, 8.0)
T = 25
NB_MAX = 40
SHAPES = [(8, 21), (64, 6), (100, 3)]  # several envs per wave + a partial last workgroup; exact 64; two waves
STATE_KEYS = ("pos", "vel", "yaw", "pitch", "real_len", "max_dev", "extra_len", "wp_idx", "arrive", "dest")
OUT_KEYS = ("obs", "vo_count", "reward", "done", "info", "finish", "reset_mask")
FILLER = np.array([12.0, 12.0, 100.0, 30.0])  # behind counts[e]: hits everybody, if it were read
RADIUS = 0.2


# ---- inputs (no GPU needed: the CPU check of the docstring's table imports them) ---------------------------------------

@functools.lru_cache(maxsize=None)
def building_sets(N):
    rng = np.random.default_rng(100 + N)

    def draw(n):
        return np.stack([rng.uniform(2, 22, n), rng.uniform(2, 22, n), rng.uniform(0.5, 9, n),
                         rng.uniform(0.05, 1.5, n)], axis=1)

    A = np.zeros((0, 4))
    B = draw(10)
    c1, c2 = draw(20), draw(20)
    c2[:, 0] = rng.uniform(9, 14, 20)  # 20 buildings inside one 8 m cell
    c2[:, 1] = rng.uniform(9, 14, 20)
    return A, B, np.concatenate([c1, c2])


@functools.lru_cache(maxsize=None)
def patrols(N):
    """Per set: (endpoint 1 [n, 2], speed [n]).  The segment from a building to its endpoint 1 leaves the building's cell."""
    rng = np.random.default_rng(300 + N)
    out = []
    for k, s in enumerate(building_sets(N)):
        n = len(s)
        e1 = np.empty((n, 2))
        for b in range(n):
            while True:
                e1[b] = rng.uniform(1, 23, 2)
                if k == 2 and b >= 20:  # C's cluster patrols to the corners of the map: the centre cell empties
                    e1[b] = np.where(rng.uniform(0, 1, 2) < 0.5, rng.uniform(1, 4, 2), rng.uniform(20, 23, 2))
                if ref.cell_of(e1[b, 0], e1[b, 1], 3, 3) != ref.cell_of(s[b, 0], s[b, 1], 3, 3):
                    break
        speed = rng.uniform(0.3, 1.5, n)
        speed[6::7] = 0.0
        out.append((e1, speed))
    return out


@functools.lru_cache(maxsize=None)
def inputs(N, E):
    """(the per-env world, ends [E, 40, 2, 2], speed [E, 40]); the fillers' ends are zeros and their speed is 9: they
    would show if they moved."""
    base = synthetic_world(E, N, MAP, min_sep=0.8, seed=41)
    sets, pat = building_sets(N), patrols(N)
    bld = np.empty((E, NB_MAX, 4))
    bld[:] = FILLER
    cnt = np.zeros(E, np.int32)
    ends, speed = np.zeros((E, NB_MAX, 2, 2)), np.full((E, NB_MAX), 9.0)
    for e in range(E):
        s, (e1, sp) = sets[e % 3], pat[e % 3]
        n = len(s)
        bld[e, :n], cnt[e] = s, n
        ends[e, :n, 0], ends[e, :n, 1], speed[e, :n] = s[:, :2], e1, sp
    return World(base.waypoints, base.n_points, base.map_size, bld, cnt), ends, speed


@functools.lru_cache(maxsize=None)
def trajectory(N, E, steps=T, mask=None):
    """The numpy reference: positions[t] [E, 40, 4] after t steps (the fillers as the caller's array has them) and leg[t]."""
    world, ends, speed = inputs(N, E)
    live = np.arange(NB_MAX)[None, :] < world.building_counts[:, None]
    rec = world.buildings.copy()
    rec[~live, 2] = -np.inf  # what the handle holds behind counts[e]
    leg = np.ones((E, NB_MAX), np.uint8)
    pos, legs = [world.buildings.copy()], [leg]
    for t in range(steps):
        rec, leg = ref.move(rec, ends, speed, leg, 1.0, None if mask is None else np.array(mask))
        p = rec.copy()
        p[~live] = FILLER
        pos.append(p); legs.append(leg)
    return pos, legs


def movement_tally(N, E):
    """(buildings per set that change their cell at least once, steps in which C's centre cell overflows, steps it does not)"""
    world, _, _ = inputs(N, E)
    pos, _ = trajectory(N, E)
    movers = []
    for s in (1, 2):
        e, n = s, int(world.building_counts[s])
        cells = np.stack([ref.cell_of(p[e, :n, 0], p[e, :n, 1], 3, 3) for p in pos])
        movers.append(int((cells != cells[0]).any(0).sum()))
    over = [int(ref.list_lengths(p[2, :40], RADIUS, 3, 3)[4] > 15) for p in pos[1:]]
    return movers, sum(over), len(over) - sum(over)


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def host(t):
    return t.cpu().numpy()


def same(a, b, what):
    a, b = host(a), host(b)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what


def assert_handles_equal(a, b, what, state=True):
    for k in OUT_KEYS:
        same(getattr(a, k), getattr(b, k), f"{what}: {k}")
    if state:
        sa, sb = a.get_state(), b.get_state()
        for k in STATE_KEYS:
            same(sa[k], sb[k], f"{what}: state {k}")


def assert_readers_equal(a, b, what):
    sa, sb = a.safety(), b.safety()
    for k, name in enumerate(("sep", "bclear", "wall", "near_pairs")):
        same(sa[k], sb[k], f"{what}: safety {name}")
    ra, rb = a.building_rows(k=4), b.building_rows(k=4)
    same(ra[0], rb[0], f"{what}: building rows")
    same(ra[1], rb[1], f"{what}: b_count")


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def assert_live_positions(motion, world, want, what):
    """M's device_buildings: the live records bit for bit the reference's, the fillers never written."""
    got = host(motion.buildings)
    live = np.arange(NB_MAX)[None, :] < world.building_counts[:, None]
    assert bits_equal(got[live], want[live]), what
    assert bits_equal(got[~live], np.broadcast_to(FILLER, got[~live].shape)), what + ": fillers"


@functools.lru_cache(maxsize=None)
def run(N, E, autoreset):
    """M (motion attached), H (the reference's positions through set_env_buildings before every step) and S (the same
    sets, static) over the same actions, M against H after every step; returns the tallies the tests assert on."""
    world, ends, speed = inputs(N, E)
    pos, legs = trajectory(N, E)
    M, H, S = (BatchedDroneEnv(world, radius=RADIUS) for _ in range(3))
    motion = BuildingMotion(ends, speed, dt=1.0)
    M.attach_building_motion(motion)
    envs = (M, H, S)
    for x in envs:
        x.observe()
    assert_handles_equal(M, H, "start")
    of_set = [np.arange(s, E, 3) for s in range(3)]
    tally = dict(done=0, flags=[0, 0, 0], bclear_diff=0)
    for t in range(T):
        a = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        H.set_env_buildings(pos[t + 1], world.building_counts)
        for x in envs:
            x.step(a, autoreset=autoreset)
        what = f"{N}x{E} autoreset={autoreset} step {t}"
        assert_handles_equal(M, H, what)
        bld, cnt = M.device_buildings()
        assert bld is motion.buildings and np.array_equal(host(cnt), world.building_counts)
        assert_live_positions(motion, world, pos[t + 1], what)
        assert np.array_equal(host(motion.leg), legs[t + 1]), what + ": leg"
        done, static = host(M.done).astype(bool), host(S.done).astype(bool)
        tally["done"] += int(done.sum())
        for s in range(3):
            tally["flags"][s] += int((done[of_set[s]] != static[of_set[s]]).sum())
        if not autoreset:
            assert_readers_equal(M, H, what)
            tally["bclear_diff"] += int((host(M.safety()[1]) != host(S.safety()[1])).sum())
            for x in envs:
                x.reset_drones(x.done | x.finish)
                x.observe()
            assert_handles_equal(M, H, what + ", after the resets")
    for x in envs:
        x.close()
    print(f"{N}x{E} autoreset={autoreset}: {tally}")
    return tally


# ---- 1. moved on the device == set from the host ------------------------------------------------------------------------

@pytest.mark.parametrize("N,E", SHAPES)
@pytest.mark.parametrize("autoreset", [True, False])
def test_moved_on_the_device_equals_set_from_the_host(N, E, autoreset):
    """obs, vo_count, reward, done, info, finish, reset_mask and every state key after every step - with the fused
    auto-reset step, and with step + reset_drones(done | finish) + observe -, and M's device_buildings() against the
    reference's positions bit for bit."""
    tally = run(N, E, autoreset)
    assert tally["done"] > 0, tally


def test_records_beyond_the_lds_cap():
    """nb_max 1100: the kernel keeps (x, y, reach) of the first 512 records in LDS and reads the others back from the
    records it has just written.  The first 1030 records stand still far outside the map (they fill the unbounded corner
    cell, which overflows, and no other), so every other cell's list is made of records beyond the cap; 70 of them
    patrol inside the map.  M against H as above, 8 steps, envs with 1100 / 1040 / 0 records."""
    N, E, nb, far = 8, 3, 1100, 1030
    base = synthetic_world(E, N, MAP, min_sep=0.8, seed=41)
    rng = np.random.default_rng(77)
    bld = np.empty((E, nb, 4))
    bld[:, :, 0], bld[:, :, 1], bld[:, :, 2], bld[:, :, 3] = -50.0, -50.0, 5.0, 0.5
    n_in = nb - far
    bld[:, far:] = np.stack([rng.uniform(2, 22, (E, n_in)), rng.uniform(2, 22, (E, n_in)), rng.uniform(0.5, 9, (E, n_in)),
                             rng.uniform(0.05, 1.5, (E, n_in))], axis=2)
    cnt = np.array([nb, 1040, 0], np.int32)
    ends, speed = np.zeros((E, nb, 2, 2)), np.zeros((E, nb))
    ends[:, :, 0] = bld[:, :, :2]
    ends[:, :, 1] = rng.uniform(1, 23, (E, nb, 2))
    speed[:, far:] = rng.uniform(0.3, 1.5, (E, n_in))
    world = World(base.waypoints, base.n_points, base.map_size, bld, cnt)
    live = np.arange(nb)[None, :] < cnt[:, None]
    rec = bld.copy()
    rec[~live, 2] = -np.inf
    leg = np.ones((E, nb), np.uint8)
    M, H = BatchedDroneEnv(world, radius=RADIUS), BatchedDroneEnv(world, radius=RADIUS)
    motion = BuildingMotion(ends, speed)
    M.attach_building_motion(motion)
    M.observe(); H.observe()
    lengths, done = [], 0
    for t in range(8):
        rec, leg = ref.move(rec, ends, speed, leg, 1.0)
        pos = np.where(live[..., None], rec, bld)
        lengths.append(ref.list_lengths(pos[1, :1040], RADIUS, 3, 3))
        H.set_env_buildings(pos, cnt)
        a = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        M.step(a); H.step(a)
        assert_handles_equal(M, H, f"step {t}")
        assert_readers_equal(M, H, f"step {t}")
        assert bits_equal(host(motion.buildings)[live], pos[live]) and np.array_equal(host(motion.leg), leg)
        done += int(host(M.done).sum())
        for x in (M, H):
            x.reset_drones(x.done | x.finish)
            x.observe()
    lengths = np.stack(lengths)
    assert (lengths[:, 0] > 15).all() and (lengths[:, 1:] <= 15).all() and (lengths[:, 1:] > 0).any(), lengths
    assert (lengths[1:, 1:] != lengths[:-1, 1:]).any()  # the lists of the other cells change
    assert done > 0
    M.close(); H.close()


# ---- 2. not vacuous -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,E", SHAPES)
def test_the_motion_matters(N, E):
    """Buildings of B and of C change their cell, C's centre cell overflows in some steps and not in others (the lists'
    lengths by brute force on the reference's positions), and the done flags inside the envs of B and of C differ from
    the handle whose sets stand still (A's never do: it has no buildings)."""
    movers, over, under = movement_tally(N, E)
    assert movers[0] >= 1 and movers[1] >= 1, movers
    assert over >= 1 and under >= 1, (over, under)
    tally = run(N, E, False)
    assert tally["flags"][0] == 0 and tally["flags"][1] > 0 and tally["flags"][2] > 0, tally
    assert tally["bclear_diff"] > 0, tally


# ---- 3. masking ---------------------------------------------------------------------------------------------------------

def test_env_mask_moves_only_the_masked_envs():
    """Three masked launches: the masked envs' records, leg and buildings_out are the reference's, the others keep their
    bits; then, with the motion detached (the records stay where they are), M steps like a handle that was given those
    positions."""
    N, E = 8, 21
    world, ends, speed = inputs(N, E)
    mask = tuple(int(e % 2 or e == 8) for e in range(E))  # envs of all three sets on either side
    pos, legs = trajectory(N, E, 3, mask)
    m = np.array(mask, bool)
    assert not bits_equal(pos[3][m], pos[0][m]) and bits_equal(pos[3][~m], pos[0][~m])
    M, H = BatchedDroneEnv(world, radius=RADIUS), BatchedDroneEnv(world, radius=RADIUS)
    motion = BuildingMotion(ends, speed)
    M.attach_building_motion(motion)
    for t in range(3):
        motion.advance(torch.tensor(mask, dtype=torch.bool))
        assert_live_positions(motion, world, pos[t + 1], f"masked launch {t}")
        assert np.array_equal(host(motion.leg), legs[t + 1])
    assert np.array_equal(legs[3][~m], legs[0][~m])
    H.set_env_buildings(pos[3], world.building_counts)
    M.observe(); H.observe()
    assert_readers_equal(M, H, "after the masked launches")
    M.attach_building_motion(None)
    assert np.array_equal(host(M.device_buildings()[0]), pos[3])
    for t in range(4):
        a = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        M.step(a, autoreset=True); H.step(a, autoreset=True)
        assert_handles_equal(M, H, f"detached, step {t}")
    M.close(); H.close()


# ---- 4. readers: covered after every plain step of run(); here behind reset() / load_state_dict() --------------------------

def test_reset_and_state_dict():
    N, E = 8, 21
    world, ends, speed = inputs(N, E)
    pos, legs = trajectory(N, E)
    M, H = BatchedDroneEnv(world, radius=RADIUS), BatchedDroneEnv(world, radius=RADIUS)
    motion = BuildingMotion(ends, speed)
    M.attach_building_motion(motion)
    M.observe(); H.observe()

    def steps(t0, n):
        for t in range(t0, t0 + n):
            a = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
            H.set_env_buildings(pos[t + 1], world.building_counts)
            M.step(a, autoreset=True); H.step(a, autoreset=True)
            assert_handles_equal(M, H, f"step {t}")
            assert_readers_equal(M, H, f"step {t}")

    steps(0, 4)
    sd = motion.state_dict()
    steps(4, 3)
    motion.load_state_dict(sd)  # back to the positions after 4 steps
    assert_live_positions(motion, world, pos[4], "load_state_dict")
    state = M.get_state()
    H.set_state(**state)
    M.observe(); H.observe()
    steps(4, 3)
    motion.reset()
    assert_live_positions(motion, world, pos[0], "reset")
    assert np.array_equal(host(motion.leg), legs[0])
    H.set_state(**M.get_state())
    M.observe(); H.observe()
    steps(0, 3)
    M.close(); H.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------

def test_refused_calls_change_nothing():
    N, E = 8, 21
    world, ends, speed = inputs(N, E)
    L = _lib.lib()
    a, twin = BatchedDroneEnv(world, radius=RADIUS), BatchedDroneEnv(world, radius=RADIUS)
    dev = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).cuda()
    e_t, s_t, leg = dev(ends, torch.float64), dev(speed, torch.float64), torch.ones((E, NB_MAX), dtype=torch.uint8).cuda()
    out = torch.full((E, NB_MAX, 4), -7.0, dtype=torch.float64).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(h, args, dt=1.0):
        return L.rvo3d_move_env_buildings(h, None if args is None else C.byref(args), dt, None, p(out), None)

    ok = _lib.BuildingMotionArgs(e_t.data_ptr(), s_t.data_ptr(), leg.data_ptr())
    # no sets attached: a handle of the shared list, and one without a world
    shared = BatchedDroneEnv(World(world.waypoints, world.n_points, world.map_size, building_sets(N)[1].copy()))
    assert call(shared._h, ok) == -3 and b"rvo3d_set_env_buildings" in L.rvo3d_last_error()   # RVO3D_ERR_STATE
    cfg = _lib.Config(E, N, 2, 0, 10, 1, 0, -1, (C.c_double * 3)(*MAP))
    raw = C.c_void_p()
    _lib.check(L.rvo3d_create(C.byref(cfg), C.byref(raw)), "rvo3d_create")
    assert call(raw, ok) == -3 and b"rvo3d_load_world" in L.rvo3d_last_error()
    L.rvo3d_destroy(raw)
    assert call(None, ok) == -1                                                              # RVO3D_ERR_INVALID
    assert call(a._h, None) == -1
    for k in range(3):
        ptrs = [e_t.data_ptr(), s_t.data_ptr(), leg.data_ptr()]
        ptrs[k] = None
        assert call(a._h, _lib.BuildingMotionArgs(*ptrs)) == -1 and b"required" in L.rvo3d_last_error(), k
    for dt in (-1.0, float("nan"), float("inf")):
        assert call(a._h, ok, dt) == -1 and b"dt" in L.rvo3d_last_error(), dt
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((leg == 1).all())
    a.observe(); twin.observe()
    for t in range(4):
        act = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        a.step(act, autoreset=True); twin.step(act, autoreset=True)
        assert_handles_equal(a, twin, f"after refused calls, step {t}")
    # the Python surface
    with pytest.raises(ValueError):
        shared.attach_building_motion(BuildingMotion(ends, speed))
    with pytest.raises(ValueError):
        a.attach_building_motion(BuildingMotion(ends[:, :39], speed[:, :39]))
    with pytest.raises(ValueError):
        BuildingMotion(np.where(np.arange(4).reshape(2, 2) == 3, np.nan, ends), speed)
    with pytest.raises(ValueError):
        BuildingMotion(ends, speed, dt=-1.0)
    motion = BuildingMotion(ends, speed)
    a.attach_building_motion(motion)
    a.set_env_buildings(world.buildings, world.building_counts)  # detaches
    assert a._motion is None and a.device_buildings()[0] is not motion.buildings
    for x in (a, twin, shared):
        x.close()


def test_graph_rollout_with_a_motion_raises():
    from rvo3d_amd.policy import mlp_ac, multi_ppo
    N, E = 8, 6
    world, ends, speed = inputs(N, E)
    env = BatchedDroneEnv(world)
    torch.manual_seed(0)
    ac = mlp_ac(env.W).cuda()
    env.attach_building_motion(BuildingMotion(ends, speed))
    with pytest.raises(ValueError, match="graph_rollout"):
        multi_ppo(env, ac, steps_per_epoch=4, max_ep_len=9, graph_rollout=True)
    env.attach_building_motion(None)
    tr = multi_ppo(env, ac, steps_per_epoch=4, max_ep_len=9, train_pi_iters=1, train_v_iters=1, amp=True, graph_rollout=True)
    env.attach_building_motion(BuildingMotion(ends, speed))  # attached behind the trainer's back
    env.reset(); env.observe()
    with pytest.raises(ValueError, match="graph_rollout"):
        tr.collect()
    env.close()


# ---- 6. trainer ---------------------------------------------------------------------------------------------------------

def test_one_training_epoch_with_moving_buildings():
    """multi_ppo on a BuildingObsEnv with synthetic_patrols attached: one epoch of 8 steps (the stream path) runs to the end,
    the parameters change, and the buildings are not where they started."""
    from rvo3d_amd.policy import mlp_ac, multi_ppo
    N, E = 8, 6
    world, _, _ = inputs(N, E)
    env = BuildingObsEnv(world, building_rows=4)
    motion = synthetic_patrols(world, seed=5, speed=(0.3, 1.5), span=6.0)
    assert motion.shape == (E, NB_MAX)
    env.attach_building_motion(motion)
    start = host(env.device_buildings()[0]).copy()
    torch.manual_seed(1)
    ac = mlp_ac(env.W).cuda()
    tr = multi_ppo(env, ac, steps_per_epoch=8, max_ep_len=50, train_pi_iters=1, train_v_iters=1, seed=3)
    env.reset(); env.observe()
    before = [q.detach().clone() for q in ac.parameters()]
    assert np.isfinite(tr.collect())
    assert tr.buf.ptr == 8
    tr.update(tr.buf.get())
    assert any(not torch.equal(x, y) for x, y in zip(before, ac.parameters()))
    now = host(env.device_buildings()[0])
    live = np.arange(NB_MAX)[None, :] < world.building_counts[:, None]
    # one launch per env step: where the numpy reference is after 8 steps, bit for bit.  (Not every building is away from
    # its start: a patrol of 1, 2 or 4 steps per leg is back there after 8.)
    rec, leg = start.copy(), np.ones((E, NB_MAX), np.uint8)
    rec[~live, 2] = -np.inf
    for t in range(8):
        rec, leg = ref.move(rec, host(motion.ends), host(motion.speed), leg, 1.0)
    assert bits_equal(now[live], rec[live]) and np.array_equal(host(motion.leg), leg)
    assert (now[live][:, :2] != start[live][:, :2]).any(1).mean() > 0.5
    assert bits_equal(now[~live], start[~live])
    env.close()
