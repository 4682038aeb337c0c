"""Per-env building sets (rvo3d_set_env_buildings; World.buildings [E, nb_max, 4]) on the GPU.

The yardstick is the shared-list path, which test_gpu_parity.py pins to the reference: env e of a handle with per-env
sets must behave bit for bit as env e of a handle whose shared list is env e's list - the same kernel, the same
arithmetic.  A numpy restatement of the building test checks the flags independently of the shared path, and further
tests make sure the comparison is not vacuous: the sets change the flags, and set C's cells have short lists, lists
walked from memory and an overflowing list (the three paths of building_hit).

Inputs: map (24, 24, 8), synthetic_world(E, N, map, min_sep=0.8, seed=41), synthetic_actions(E, N, t, 1234), 25 steps.
Env e gets set e % 3: A empty, B 10 buildings, C 40 buildings of which 20 sit inside one 8 m cell.  The same inputs on
the CPU oracle, stepped without auto-reset, gave (hits inside the envs of B / of C, done flags there that differ from
a world without buildings):

    N x E     B hits  C hits  B flags  C flags
    8 x 21        56     162       75      183
    16 x 13      135     179      165      194
    48 x 6        47     247       66      286
    64 x 6       117     482      151      552
    100 x 3       76     398       95      443
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, World, _lib, synthetic_actions, synthetic_world

pytestmark = pytest.mark.gpu

MAP = (24.0, 24.0, 8.0)
T = 25
SHAPES = [(8, 21), (16, 13), (48, 6), (64, 6), (100, 3)]  # several envs per wave + a partial last workgroup (x2);
#                                                             padded kernel with ghost lanes; exact 64; two waves
STATE_KEYS = ("pos", "vel", "yaw", "pitch", "real_len", "max_dev", "extra_len", "wp_idx", "arrive", "dest")


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


def worlds_of(N, E, rot=0):
    """(per-env world: env e holds set (e + rot) % 3 - counts 0 / 10 / 40, nb_max 40, the unused records filled with a
    building in the middle of the map that must never be seen -, [the same routes with A / B / C shared])"""
    base = synthetic_world(E, N, MAP, min_sep=0.8, seed=41)
    sets = building_sets(N)
    bld = np.empty((E, 40, 4))
    bld[:] = np.array([12.0, 12.0, 100.0, 30.0])  # hits everybody, if it were read
    cnt = np.zeros(E, np.int32)
    for e in range(E):
        s = sets[(e + rot) % 3]
        bld[e, :len(s)] = s
        cnt[e] = len(s)
    per = World(base.waypoints, base.n_points, base.map_size, bld, cnt)
    shared = [World(base.waypoints, base.n_points, base.map_size, s.copy()) for s in sets]
    return per, shared


def radii(N, E):
    return np.round(np.random.default_rng(7 + N).uniform(0.1, 0.9, (E, N)), 2)


def host(t):
    return t.cpu().numpy()


def assert_envs_equal(a, b, envs, what):
    """np.array_equal of two arrays' rows `envs`, NaN == NaN for floats: no tolerance."""
    a, b = host(a)[envs], host(b)[envs]
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what


def compare(per, shared, E, rot, what, state=True):
    for s in range(3):
        envs = np.array([e for e in range(E) if (e + rot) % 3 == s], dtype=np.int64)
        for k in ("obs", "reward", "vo_count", "done", "info", "finish", "reset_mask"):
            assert_envs_equal(getattr(per, k), getattr(shared[s], k), envs, f"{what}: {k} of set {'ABC'[s]}")
        if state:
            sp, ss = per.get_state(), shared[s].get_state()
            for k in STATE_KEYS:
                assert_envs_equal(sp[k], ss[k], envs, f"{what}: state {k} of set {'ABC'[s]}")


def building_hits(pos, bld_of_env, radius):
    """The building test in float64 numpy, per drone against its own env's list (rvo_inter.py:99-105, 198-209).
    Returns (hit [E, N], robust hit [E, N]: away from both thresholds by 1e-9, pairs inside a 1e-9 band)."""
    E, N = pos.shape[:2]
    hit, robust = np.zeros((E, N), bool), np.zeros((E, N), bool)
    knife = 0
    r = np.broadcast_to(np.asarray(radius, dtype=np.float64), (E, N))
    for e in range(E):
        b = bld_of_env(e)
        if len(b) == 0:
            continue
        ex = pos[e, :, None, 0] - b[None, :, 0]
        ey = pos[e, :, None, 1] - b[None, :, 1]
        z, h, reach = pos[e, :, None, 2], b[None, :, 2], r[e, :, None] + b[None, :, 3]
        dis = np.sqrt(ex ** 2 + ey ** 2)
        height = (h > z - 2) & (z <= h)
        m = height & (dis <= 5) & (dis <= reach)
        edge = (np.abs(dis - reach) <= 1e-9) | (np.abs(dis - 5) <= 1e-9)
        knife += int((height & edge).sum())
        hit[e] = m.any(1)
        robust[e] = (m & ~edge).any(1)
    return hit, robust, knife


@functools.lru_cache(maxsize=None)
def run(N, E, autoreset, per_drone_radius=False):
    """One per-env handle next to three shared-list handles over the same E envs, compared every step; returns the
    tallies the other tests assert on (computed once per shape)."""
    per_w, shared_w = worlds_of(N, E)
    radius = radii(N, E) if per_drone_radius else 0.2
    per = BatchedDroneEnv(per_w, radius=radius)
    shared = [BatchedDroneEnv(w, radius=radius) for w in shared_w]
    envs = [per] + shared
    for x in envs:
        x.observe()
    compare(per, shared, E, 0, "start")
    tally = dict(hits=[0, 0, 0], flags=[0, 0, 0], missed=0, knife=0, done=0)
    of_set = [np.arange(s, E, 3) for s in range(3)]
    for t in range(T):
        a = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        for x in envs:
            x.step(a, autoreset=autoreset)
        compare(per, shared, E, 0, f"{N}x{E} step {t}")
        done = host(per.done).astype(bool)
        tally["done"] += int(done.sum())
        if not autoreset:
            # the post-step positions, against each drone's own env's list
            hit, robust, knife = building_hits(host(per.get_state()["pos"]), per_w.env_buildings, radius)
            tally["missed"] += int((robust & ~done).sum())
            tally["knife"] += knife
            none = host(shared[0].done).astype(bool)
            for s in (1, 2):
                tally["hits"][s] += int(hit[of_set[s]].sum())
                tally["flags"][s] += int((done[of_set[s]] != none[of_set[s]]).sum())
            assert not hit[of_set[0]].any()
            for x in envs:
                x.reset_drones(x.done | x.finish)
                x.observe()
            compare(per, shared, E, 0, f"{N}x{E} step {t}, after the resets")
    for x in envs:
        x.close()
    print(f"{N}x{E} autoreset={autoreset} radii={per_drone_radius}: {tally}")
    return tally


@pytest.mark.parametrize("N,E", SHAPES)
@pytest.mark.parametrize("autoreset", [True, False])
def test_per_env_sets_equal_shared_lists_bit_for_bit(N, E, autoreset):
    """Env e of the per-env handle against env e of the shared-list handle of set e % 3 (no buildings, list B, list C):
    obs, reward, vo_count, done, info, finish, reset_mask and the whole state, every step - with the fused auto-reset
    step, and with step + reset_drones(done | finish) + observe."""
    tally = run(N, E, autoreset)
    assert tally["done"] > 0, tally


def test_per_env_sets_with_per_drone_radii():
    """16 x 13 again with radii round(U(0.1, 0.9), 2): the lists' reach uses the largest radius of the handle.
    Building hits inside the envs of B / C in the run without auto-reset: 191 / 304."""
    for autoreset in (True, False):
        tally = run(16, 13, autoreset, True)
        assert tally["done"] > 0, tally
    assert tally["hits"][1] > 0 and tally["hits"][2] > 0, tally
    assert tally["missed"] == 0 and tally["knife"] == 0, tally


@pytest.mark.parametrize("N,E", SHAPES)
def test_the_sets_matter(N, E):
    """The comparison cannot pass vacuously: inside the envs of B and of C drones hit buildings (the numpy restatement
    on the post-step positions), and their done flags differ from the handle without buildings."""
    tally = run(N, E, False)
    for s in (1, 2):
        assert tally["hits"][s] > 0 and tally["flags"][s] > 0, tally


@pytest.mark.parametrize("N", [n for n, _ in SHAPES])
def test_set_C_reaches_all_three_list_paths(N):
    """The per-cell list lengths of set C, restated by brute force (a building is listed where a drone of the largest
    radius inside the cell, widened by 1e-3 m and unbounded at the map's edge, could touch it within the 5 m gate):
    cells with 1..4 entries (tested from the first load), 5..15 (walked from memory), more than 15 (overflow: every
    building is tested)."""
    Cset = building_sets(N)[2]
    cs, n = 8.0, 3  # 24 m / 8 m cells
    lengths = []
    for rmax in (0.2, 0.9):
        for ix in range(n):
            for iy in range(n):
                x0, x1 = (-np.inf if ix == 0 else ix * cs), (np.inf if ix == n - 1 else (ix + 1) * cs)
                y0, y1 = (-np.inf if iy == 0 else iy * cs), (np.inf if iy == n - 1 else (iy + 1) * cs)
                dx = np.where(Cset[:, 0] < x0, x0 - Cset[:, 0], np.where(Cset[:, 0] > x1, Cset[:, 0] - x1, 0.0))
                dy = np.where(Cset[:, 1] < y0, y0 - Cset[:, 1], np.where(Cset[:, 1] > y1, Cset[:, 1] - y1, 0.0))
                reach = np.minimum(rmax + Cset[:, 3], 5.0) + 1e-3
                lengths.append(int((dx * dx + dy * dy <= reach * reach).sum()))
        assert any(1 <= k <= 4 for k in lengths[-9:]), lengths
        assert any(5 <= k <= 15 for k in lengths[-9:]), lengths
        assert any(k > 15 for k in lengths[-9:]), lengths


@pytest.mark.parametrize("N,E", SHAPES)
def test_flags_agree_with_a_numpy_restatement_of_the_building_test(N, E):
    """Independent of the shared path: wherever (h > z - 2) & (dis <= 5) & (z <= h) & (dis <= r + br) holds for a
    drone's post-step position and a building of its own env, away from both thresholds by more than 1e-9, done is
    set.  No pair is expected inside the 1e-9 band (the CPU oracle's smallest |dis - (r + br)| was 6.5e-6)."""
    tally = run(N, E, False)
    assert tally["missed"] == 0, tally
    assert tally["knife"] == 0, tally


# ---- the contract of rvo3d_set_env_buildings ---------------------------------------------------------------------------

def steps_equal(a, b, n, N, E, t0=0, what=""):
    for t in range(t0, t0 + n):
        act = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        a.step(act, autoreset=True)
        b.step(act, autoreset=True)
        every = np.arange(E)
        for k in ("obs", "reward", "vo_count", "done", "info", "finish", "reset_mask"):
            assert_envs_equal(getattr(a, k), getattr(b, k), every, f"{what} step {t}: {k}")
        sa, sb = a.get_state(), b.get_state()
        for k in STATE_KEYS:
            assert_envs_equal(sa[k], sb[k], every, f"{what} step {t}: state {k}")


def test_attach_then_detach_equals_never_attached():
    N, E = 16, 13
    per_w, shared_w = worlds_of(N, E)
    a, fresh = BatchedDroneEnv(shared_w[1]), BatchedDroneEnv(shared_w[1])
    a.set_env_buildings(per_w.buildings, per_w.building_counts)
    a.set_env_buildings(None)
    a.observe(); fresh.observe()
    steps_equal(a, fresh, 5, N, E, what="detached")
    a.close(); fresh.close()


def test_replacing_the_sets_takes_effect_on_the_next_step():
    N, E = 16, 13
    per_w, _ = worlds_of(N, E)
    new_w, new_shared_w = worlds_of(N, E, rot=1)  # env e moves on to set (e + 1) % 3
    per = BatchedDroneEnv(per_w)
    per.observe()
    for t in range(6):
        per.step(torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda(), autoreset=True)
    per.set_env_buildings(new_w.buildings, new_w.building_counts)
    state = per.get_state()
    others = [BatchedDroneEnv(new_w)] + [BatchedDroneEnv(w) for w in new_shared_w]
    for x in others:
        x.set_state(**state)
    hits = 0
    for t in range(6, 12):
        a = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        for x in [per] + others:
            x.step(a, autoreset=True)
        steps = f"replaced, step {t}"
        for k in ("obs", "reward", "vo_count", "done", "info", "finish", "reset_mask"):
            assert_envs_equal(getattr(per, k), getattr(others[0], k), np.arange(E), f"{steps}: {k}")
        compare(per, others[1:], E, 1, steps)
        hits += int(host(per.done).sum())
    assert hits > 0
    for x in [per] + others:
        x.close()


def raw_handle(E, N, P=2, nb=0):
    cfg = _lib.Config(E, N, P, nb, 10, 1, 0, -1, (C.c_double * 3)(*MAP))
    h = C.c_void_p()
    _lib.check(_lib.lib().rvo3d_create(C.byref(cfg), C.byref(h)), "rvo3d_create")
    return h


def test_needs_a_loaded_world():
    L = _lib.lib()
    h = raw_handle(3, 8)
    b = np.zeros((3, 2, 4))
    assert L.rvo3d_set_env_buildings(h, C.c_void_p(b.ctypes.data), None, 2, None) == -3  # RVO3D_ERR_STATE
    assert b"rvo3d_load_world" in L.rvo3d_last_error()
    assert L.rvo3d_set_env_buildings(None, C.c_void_p(b.ctypes.data), None, 2, None) == -1
    L.rvo3d_destroy(h)


def test_refused_calls_leave_the_handle_as_it_was():
    N, E = 16, 13
    per_w, _ = worlds_of(N, E)
    a, twin = BatchedDroneEnv(per_w), BatchedDroneEnv(per_w)
    L = _lib.lib()
    bld = np.ascontiguousarray(per_w.buildings)
    bp = C.c_void_p(bld.ctypes.data)

    def call(counts, nb_max, buildings=bp):
        c = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
        return L.rvo3d_set_env_buildings(a._h, buildings, None if c is None else C.c_void_p(c.ctypes.data), nb_max, None)

    neg, over = per_w.building_counts.copy(), per_w.building_counts.copy()
    neg[E - 1] = -1
    over[0] = 41
    assert call(neg, 40) == -1 and b"counts" in L.rvo3d_last_error()   # RVO3D_ERR_INVALID
    assert call(over, 40) == -1
    assert call(None, 0xffff) == -1 and b"nb_max" in L.rvo3d_last_error()
    assert call(None, 1 << 20) == -1
    assert call(None, -1) == -1
    with pytest.raises(_lib.RVO3DError):
        a.set_env_buildings(per_w.buildings, over)
    with pytest.raises(AssertionError):
        a.set_env_buildings(per_w.buildings[:, :, :3])
    a.observe(); twin.observe()
    steps_equal(a, twin, 5, N, E, what="after refused calls")
    a.close(); twin.close()


def test_load_world_again_drops_the_sets():
    N, E = 16, 13
    per_w, shared_w = worlds_of(N, E)
    a, none = BatchedDroneEnv(per_w), BatchedDroneEnv(shared_w[0])
    wp = np.ascontiguousarray(per_w.waypoints, dtype=np.float64)
    npts = np.ascontiguousarray(per_w.n_points, dtype=np.int32)
    _lib.check(_lib.lib().rvo3d_load_world(a._h, C.c_void_p(wp.ctypes.data), C.c_void_p(npts.ctypes.data), None, None, None,
                                           None), "rvo3d_load_world")
    a.observe(); none.observe()
    steps_equal(a, none, 5, N, E, what="reloaded")
    # and they can be attached again
    b = BatchedDroneEnv(per_w)
    a.set_env_buildings(per_w.buildings, per_w.building_counts)
    a.reset(); a.observe(); b.observe()
    steps_equal(a, b, 5, N, E, what="attached again")
    for x in (a, none, b):
        x.close()


# ---- Python routing ------------------------------------------------------------------------------------------------------

def test_multi_ppo_collect_is_the_same_on_a_per_env_copy_of_a_shared_list():
    """A per-env world in which every env holds the shared world's list: bit-identical collect() buffers with the same
    seed (16 drones x 8 envs, 4 steps, the MLP actor-critic, the default fused rollout)."""
    from rvo3d_amd.policy import mlp_ac, multi_ppo
    N, E, steps = 16, 8, 4
    shared_w = synthetic_world(E, N, MAP, min_sep=0.8, seed=41)
    shared_w.buildings = building_sets(N)[2].copy()
    per_w = World(shared_w.waypoints, shared_w.n_points, shared_w.map_size, np.repeat(shared_w.buildings[None], E, 0).copy())
    bufs = []
    for w in (shared_w, per_w):
        env = BatchedDroneEnv(w)
        torch.manual_seed(0)
        ac = mlp_ac(env.W).cuda()
        tr = multi_ppo(env, ac, steps_per_epoch=steps, max_ep_len=9, train_pi_iters=1, train_v_iters=1, seed=3)
        env.reset(); env.observe()
        tr.collect()
        assert tr.buf.ptr == steps
        bufs.append({k: host(getattr(tr.buf, k)).copy() for k in ("obs", "cnt", "act", "rew", "val", "logp", "cut")})
        env.close()
    for k, v in bufs[0].items():
        assert np.array_equal(v, bufs[1][k], equal_nan=v.dtype.kind == "f"), k
    assert np.abs(bufs[0]["rew"]).sum() > 0


def test_mdin_reports_and_steps_env_0s_list():
    from rvo3d_amd.drone_envs.mdin import mdin
    N = 16
    base = synthetic_world(1, N, MAP, min_sep=0.8, seed=41)
    Cset = building_sets(N)[2]
    bld = np.zeros((1, 45, 4))
    bld[0, :40] = Cset
    bld[0, 40:] = np.array([12.0, 12.0, 100.0, 30.0])
    per = mdin(world=World(base.waypoints, base.n_points, base.map_size, bld, np.array([40], np.int32)))
    shared = mdin(world=World(base.waypoints, base.n_points, base.map_size, Cset.copy()))
    assert per.ir_gym.building_list == Cset.tolist() == shared.ir_gym.building_list
    op, os_ = per.drone_reset(False), shared.drone_reset(False)
    assert all(np.array_equal(x, y) for x, y in zip(op, os_))
    dones = 0
    for t in range(12):
        act = list(synthetic_actions(1, N, t, 1234)[0])
        rp, rs = per.drone_step(act), shared.drone_step(act)
        assert all(np.array_equal(x, y) for x, y in zip(rp[0], rs[0])), t
        assert np.array_equal(np.asarray(rp[1]), np.asarray(rs[1]), equal_nan=True), t
        assert rp[2:] == rs[2:], t
        dones += sum(rp[2])
        for i in [i for i, d in enumerate(rp[2]) if d]:
            per.drone_reset_one(False, i)
            shared.drone_reset_one(False, i)
    assert dones > 0
    per.close(); shared.close()
