"""Safety metrics on the device (include/rvo3d.h: rvo3d_safety_scan, rvo3d_eval_account_safety): the scan against its numpy
restatement (rvo3d_amd.safety.safety_numpy) bit for bit over every launch geometry and building set-up, its argument
contract, counted handles, the three predicates against the step's own `done`, and the episode records of the fused
evaluation loop.  The shapes and what each is there for stand next to SHAPES; the counted scans (counted_scan) run at
(4, 130) with per-env building sets and at (70, 4), shared list and per-env sets."""
import ctypes as C

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, World, _lib, crossing_world, stack_worlds, synthetic_actions, synthetic_world
from rvo3d_amd.policy import post_train
from rvo3d_amd.safety import fold_safety_step, new_safety_run, safety_numpy
from test_safety_host import excluded_rows

pytestmark = pytest.mark.gpu
MAP = (20.0, 16.0, 8.0)
INF = np.inf
# (E, N): a sole drone, packed envs, more envs than one workgroup packs (64 at 4 lanes per env), every ring width, more
# than one wave per env, and the widest workgroup (N = 512: eight waves feed the LDS fold over waves).
# Counted handles run at (4, 130) - counts 130, 65, 64, 1: waves of ghosts alone in the fold, a wave with one live lane, an
# env of a single drone, with per-env building sets - and packed at (70, 4) with counts cycling 4, 1, 3, 2.
SHAPES = [(5, 1), (3, 2), (70, 4), (7, 33), (4, 64), (3, 65), (2, 130), (2, 257), (1, 512)]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def planted_state(E, N, seed):
    """Random positions in (and a little outside) the map with random radii, plus the edge cases: in env 0 a pair with
    dis == r_i + r_j exactly, a drone on a map face and one just outside; in the last env a drone at z = 2.0 (a planted
    building's h) and one at nextafter(2.0, inf)."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.02, 1.02, (E, N, 3)) * np.array(MAP)
    rad = np.round(rng.uniform(0.1, 0.4, (E, N)), 3)
    pos[0, 0] = [1.0, 1.0, 1.0]
    rad[0, 0] = 0.25
    if N >= 2:
        pos[0, 1] = [1.5, 1.0, 1.0]
        rad[0, 1] = 0.25
    if N >= 4:
        pos[0, 2] = [0.0, 5.0, 3.0]                       # on the face x = 0
        pos[0, 3] = [7.0, np.nextafter(MAP[1], INF), 3.0]   # just outside y = map_y
    pos[E - 1, N - 1] = [9.0, 9.0, 2.0]
    if N >= 2:
        pos[E - 1, N - 2] = [9.5, 9.0, np.nextafter(2.0, INF)]
        # a crowded env (512 drones): a random drone that touches the planted pair would hide its sep == 0; it goes 3 m up
        for j in range(2, N):
            if min(np.linalg.norm(pos[0, j] - pos[0, i]) - (rad[0, j] + 0.25) for i in (0, 1)) <= 0.0:
                pos[0, j, 2] += 3.0
    return pos, rad


def buildings_for(kind, E, seed):
    """(buildings, building_counts) of the three set-ups; the first record is the planted one (h = 2.0 next to the drones
    planted at z = 2.0)."""
    rng = np.random.default_rng(seed + 100)

    def draw(*shape):
        return np.concatenate([rng.uniform(0, MAP[0], shape + (1,)), rng.uniform(0, MAP[1], shape + (1,)),
                               rng.uniform(0, MAP[2], shape + (1,)), rng.uniform(0.5, 1.5, shape + (1,))], axis=-1)
    if kind == "none":
        return np.zeros((0, 4)), None
    if kind == "shared":
        b = draw(3)
        b[0] = [9.0, 10.0, 2.0, 0.5]
        return b, None
    b = draw(E, 300)   # per env: more than one LDS tile at every lane count
    b[:, 0] = [9.0, 10.0, 2.0, 0.5]
    cnt = rng.integers(0, 301, E).astype(np.int32)
    cnt[0], cnt[E - 1] = 0, 300
    return b, cnt


def make_env(E, N, bld, cnt, rad, drone_counts=None):
    wp = np.zeros((E, N, 2, 3))
    wp[:, :, 0] = [1.0, 1.0, 1.0]
    wp[:, :, 1] = [5.0, 5.0, 5.0]
    w = World(wp, np.full((E, N), 2, np.int32), np.array(MAP), bld, cnt, drone_counts)
    return BatchedDroneEnv(w, neighbors_num=2, radius=rad)


@pytest.mark.parametrize("E,N", SHAPES)
def test_scan_equals_the_restatement_bit_for_bit(E, N):
    pos, rad = planted_state(E, N, seed=E * 1000 + N)
    for kind in ("none", "shared", "per_env"):
        bld, cnt = buildings_for(kind, E, seed=N)
        env = make_env(E, N, bld, cnt, rad)
        env.set_state(pos=pos)
        got = [t.cpu().numpy() for t in env.safety(0.5)]
        env.close()
        want = safety_numpy(pos, rad, MAP, 0.5, buildings=bld if len(bld) else None, building_counts=cnt)
        for name, g, w in zip(("sep", "bclear", "wall"), got, want):
            bad = np.argwhere(bits(g) != bits(w))
            assert bad.size == 0, (kind, name, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]), (kind, got[3], want[3])
        # the planted cases are what they were planted for
        if N >= 2:
            assert got[0][0, 0] == 0.0 and got[0][0, 1] == 0.0
        else:
            assert np.isinf(got[0]).all()
        if N >= 4:
            assert got[2][0, 2] == 0.0 and not np.signbit(got[2][0, 2]) and got[2][0, 3] < 0
        if kind == "none":
            assert np.isinf(got[1]).all()
        else:
            assert got[1][E - 1, N - 1] <= 0.5   # the planted building counts at p_z == h: d = 1, r + r_b >= 0.6


def _scan(env, margin, sep, bclear, wall, near):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    return _lib.lib().rvo3d_safety_scan(env._h, margin, p(sep), p(bclear), p(wall), p(near), env._stream())


def _sentinels(E, N):
    f = lambda: torch.full((E, N), -7.0, dtype=torch.float64, device="cuda")
    return [f(), f(), f(), torch.full((E,), -7, dtype=torch.int32, device="cuda")]


def test_null_outputs_and_refused_arguments():
    E, N = 6, 9
    pos, rad = planted_state(E, N, seed=3)
    bld, cnt = buildings_for("shared", E, seed=3)
    env = make_env(E, N, bld, cnt, rad)
    env.set_state(pos=pos)
    full = [t.clone() for t in env.safety(0.5)]
    for k in range(4):   # each output alone: the others, pre-filled, stay as they are
        out = _sentinels(E, N)
        args = [out[i] if i == k else None for i in range(4)]
        assert _scan(env, 0.5, *args) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[k], full[k]), k
        fresh = _sentinels(E, N)
        assert all(torch.equal(out[i], fresh[i]) for i in range(4) if i != k), k
    # refused: nothing written
    out = _sentinels(E, N)
    for margin in (float("nan"), float("inf"), -float("inf"), -1e-300, -0.5):
        assert _scan(env, margin, *out) == -1, margin    # RVO3D_ERR_INVALID
        assert b"near_margin" in _lib.lib().rvo3d_last_error()
    assert _scan(env, 0.5, None, None, None, None) == -1
    assert _lib.lib().rvo3d_safety_scan(None, 0.5, *[C.c_void_p(t.data_ptr()) for t in out], env._stream()) == -1
    torch.cuda.synchronize()
    fresh = _sentinels(E, N)
    assert all(torch.equal(a, b) for a, b in zip(out, fresh))
    assert _scan(env, 0.0, *out) == 0    # (the smallest margin that is accepted)
    env.close()
    # a handle without a world: RVO3D_ERR_STATE
    L = _lib.lib()
    cfg = _lib.Config(1, 2, 2, 0, 2, 1, 0, -1, (C.c_double * 3)(*MAP))
    h = C.c_void_p()
    assert L.rvo3d_create(C.byref(cfg), C.byref(h)) == 0
    out = _sentinels(1, 2)
    assert L.rvo3d_safety_scan(h, 0.5, *[C.c_void_p(t.data_ptr()) for t in out], None) == -3
    L.rvo3d_destroy(h)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, _sentinels(1, 2)))


def test_counted_handles_equal_plain_handles():
    """A padded batch of fleets of 2 / 4 / 8 drones against plain handles of each size, on the state a few plain steps
    left: the live rows bit for bit, the ghost rows +inf; NaN in the ghosts' state changes nothing."""
    sizes, Eper = (2, 4, 8), 3
    worlds = [synthetic_world(Eper, n, (6.0, 6.0, 4.0), nb=3, seed=31, min_sep=0.5) for n in sizes]
    batch = stack_worlds(worlds, pad_drones=True)
    assert batch.drone_counts.tolist() == [2] * Eper + [4] * Eper + [8] * Eper
    N = max(sizes)
    env = BatchedDroneEnv(batch, neighbors_num=3)

    acts = [synthetic_actions(len(sizes) * Eper, N, t) for t in range(4)]
    for a in acts:
        env.step(torch.from_numpy(a).cuda())
    got = [x.cpu().numpy().copy() for x in env.safety(1.0)]
    for k, n in enumerate(sizes):
        plain = BatchedDroneEnv(worlds[k], neighbors_num=3)
        for a in acts:
            plain.step(torch.from_numpy(np.ascontiguousarray(a[k * Eper:(k + 1) * Eper, :n])).cuda())
        want = [x.cpu().numpy() for x in plain.safety(1.0)]
        plain.close()
        rows = slice(k * Eper, (k + 1) * Eper)
        for i in range(3):
            assert np.array_equal(bits(got[i][rows, :n]), bits(want[i])), (n, i)
            assert np.isposinf(got[i][rows, n:]).all(), (n, i)
        assert np.array_equal(got[3][rows], want[3]), n
    assert np.isfinite(got[0][:, :2]).all() and np.isfinite(got[2][:, :2]).all()
    # ghost state is never read
    st = env.get_state()
    pos = st["pos"].cpu().numpy()
    ghost = np.arange(N)[None, :] >= batch.drone_counts[:, None]
    pos[ghost] = np.nan
    env.set_state(pos=pos)
    again = [x.cpu().numpy() for x in env.safety(1.0)]
    for i in range(3):
        assert np.array_equal(bits(again[i]), bits(got[i])), i
    assert np.array_equal(again[3], got[3])
    # ... and the restatement agrees on the counted batch
    want = safety_numpy(pos, 0.2, batch.map_size, 1.0, counts=batch.drone_counts, buildings=batch.buildings)
    for i in range(3):
        assert np.array_equal(bits(again[i]), bits(want[i])), i
    assert np.array_equal(again[3], want[3])
    env.close()


def counted_scan(E, N, counts, kind):
    """planted_state on a counted handle with NaN in the ghosts' state against safety_numpy(counts=, building_counts=):
    live rows bit for bit, ghost rows +inf, near_pairs equal, and each of the three predicates true in some live row.
    The planted drones a count would cut away stand inside the live range: the last env's drone at z = 2.0 is its
    drone 0, the one at nextafter(2.0) the last live drone of env 1; drone 0 of env 2 stands inside the planted building."""
    counts = np.array(counts, dtype=np.int32)
    live = np.arange(N)[None, :] < counts[:, None]
    pos, rad = planted_state(E, N, seed=E * 1000 + N + 1)
    assert counts[0] >= 4 and counts[E - 1] == 1
    pos[E - 1, 0] = [9.0, 9.0, 2.0]
    pos[1, counts[1] - 1] = [9.5, 9.0, np.nextafter(2.0, INF)]
    pos[2, 0] = [9.0, 10.25, 1.5]
    pos[~live] = np.nan
    bld, cnt = buildings_for(kind, E, seed=N)
    env = make_env(E, N, bld, cnt, rad, drone_counts=counts)
    env.set_state(pos=pos)
    got = [t.cpu().numpy() for t in env.safety(0.5)]
    env.close()
    want = safety_numpy(pos, rad, MAP, 0.5, counts=counts, buildings=bld, building_counts=cnt)
    for name, g, w in zip(("sep", "bclear", "wall"), got, want):
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, (kind, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        assert np.isposinf(g[~live]).all(), (kind, name)
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]), (kind, got[3], want[3])
    assert np.isposinf(got[0][E - 1, 0]) and got[3][E - 1] == 0          # the env of one drone
    assert np.isfinite(got[0][live & (counts[:, None] > 1)]).all() and np.isfinite(got[2][live]).all()
    assert got[1][E - 1, 0] <= 0.5                                       # the planted building counts at p_z == h
    fired = [int((got[0][live] <= 0).sum()), int((got[1][live] <= 0).sum()), int((got[2][live] < 0).sum())]
    print(f"({E}, {N}) {kind}: live rows {int(live.sum())}, fired: pairs, buildings, walls {fired}, near {got[3].sum()}")
    assert min(fired) > 0 and got[3].sum() > 0


def test_counted_scan_of_several_waves_with_per_env_sets():
    counted_scan(4, 130, (130, 65, 64, 1), "per_env")


@pytest.mark.parametrize("kind", ["shared", "per_env"])
def test_counted_scan_in_the_packed_geometry(kind):
    counted_scan(70, 4, [(4, 1, 3, 2)[e % 4] for e in range(70)], kind)


def test_predicates_equal_the_steps_done():
    """Plain steps with random actions on a world of per-env building sets: after every step `done` equals
    sep <= 0 or bclear <= 0 or wall < 0 on every row, but for the rows excluded_rows names (at most 1 %); every one of
    the three predicates fires."""
    E, N, T = 6, 16, 20
    w = synthetic_world(E, N, (8.0, 8.0, 5.0), nb=6, per_env_buildings=True, seed=5, min_sep=0.6)
    env = BatchedDroneEnv(w, neighbors_num=4)
    rows = left_out = 0
    fired = np.zeros(3, dtype=np.int64)
    for t in range(T):
        _, _, _, done, _, _ = env.step(torch.from_numpy(synthetic_actions(E, N, t)).cuda())
        sep, bclear, wall, _ = (x.cpu().numpy() for x in env.safety(0.5))
        done = done.cpu().numpy().astype(bool)
        pos = env.get_state()["pos"].cpu().numpy()
        for e in range(E):
            keep = ~excluded_rows(pos[e], np.full(N, 0.2), w.buildings[e])
            pred = (sep[e] <= 0) | (bclear[e] <= 0) | (wall[e] < 0)
            assert np.array_equal(done[e][keep], pred[keep]), (t, e)
            left_out += int((~keep).sum())
        rows += E * N
        fired += [int((sep <= 0).sum()), int((bclear <= 0).sum()), int((wall < 0).sum())]
    env.close()
    print("rows", rows, "left out", left_out, "fired: pairs, buildings, walls", fired.tolist())
    assert left_out * 100 <= rows
    assert (fired > 0).all()


def _eval_world():
    """Fleets of 6 / 4 / 5 / 6 drones that start on a ring in a small map, the desired velocity as the action: drones
    pass within a metre of each other and leave the map; the envs' episodes end at different steps."""
    w = crossing_world(4, 6, (8.0, 8.0, 4.0), radius=2.5, seed=7)
    return w.with_drone_counts([6, 4, 5, 6])


def _fused(safety, **kw):
    env = BatchedDroneEnv(_eval_world(), neighbors_num=5)
    pt = post_train(env, num_episodes=8, max_ep_len=12, acceler_vel=1.0, inf_print=False, fused=True, poll_every=3,
                    safety=safety, near_margin=1.0, **kw)
    res = pt.policy_test(policy_type="des_vel")
    env.close()
    return pt, res


def test_episode_records_of_the_fused_loop():
    quota, max_ep_len, margin = 2, 12, 1.0
    pt, res = _fused(True)
    plain, res_plain = _fused(False)
    # length, return, speed, step and flags are rvo3d_eval_account's, bit for bit
    assert res == res_plain
    for k in ("rec_step", "rec_len", "rec_flags"):
        assert np.array_equal(pt.records[k], plain.records[k]), k
    for k in ("rec_ret", "rec_speed"):
        assert np.array_equal(bits(pt.records[k]), bits(plain.records[k])), k
    assert set(plain.records) == {"rec_step", "rec_len", "rec_ret", "rec_speed", "rec_flags"}
    assert len({tuple(r) for r in pt.records["rec_len"].tolist()}) > 1   # the envs end at different steps

    # a second twin: the same loop by hand, rvo3d_eval_account for the decision, env.safety() folded on the host
    env = BatchedDroneEnv(_eval_world(), neighbors_num=5)
    E = env.E
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    t = dict(ep_len=z(E, torch.int32), ep_ret=z(E, torch.float64), speed_sum=z(E, torch.float64), counted=z(E, torch.int32),
             rec_len=z((E, quota), torch.int32), rec_ret=z((E, quota), torch.float64), rec_speed=z((E, quota), torch.float64),
             rec_step=z((E, quota), torch.int64), rec_flags=z((E, quota), torch.uint8),
             remaining=torch.full((1,), E * quota, dtype=torch.int32, device="cuda"), ended=z(E, torch.uint8))
    bufs = _lib.EvalBufs(**{k: v.data_ptr() for k, v in t.items()})
    p = lambda x: C.c_void_p(x.data_ptr())
    want = dict(rec_min_sep=np.full((E, quota), INF), rec_min_bclear=np.full((E, quota), INF),
                rec_min_wall=np.full((E, quota), INF), rec_near=np.zeros((E, quota), np.int64))
    run = new_safety_run(E)
    env.reset()
    env.observe()
    step = 0
    while int(t["remaining"].item()) > 0:
        assert step < 200
        _, _, rew, done, info, fin = env.step(env.des_vel())
        fold_safety_step(run, *[x.cpu().numpy() for x in env.safety(margin)])
        counted = t["counted"].cpu().numpy().copy()
        _lib.check(_lib.lib().rvo3d_eval_account(env._h, p(rew), p(done), p(info), p(fin), max_ep_len, quota, step,
                                                 C.byref(bufs), env._stream()), "rvo3d_eval_account")
        ended = t["ended"].cpu().numpy().astype(bool)
        for e in np.nonzero(ended)[0]:
            if counted[e] < quota:
                for k, r in (("rec_min_sep", "sep"), ("rec_min_bclear", "bclear"), ("rec_min_wall", "wall"), ("rec_near", "near")):
                    want[k][e, counted[e]] = run[r][e]
            for r in ("sep", "bclear", "wall"):
                run[r][e] = INF
            run["near"][e] = 0
        env.reset(t["ended"])
        env.observe_envs(t["ended"])
        step += 1
    env.close()
    assert np.array_equal(t["rec_len"].cpu().numpy(), pt.records["rec_len"])   # the twin flew the same episodes
    for k in ("rec_min_sep", "rec_min_bclear", "rec_min_wall"):
        assert np.array_equal(bits(pt.records[k]), bits(want[k])), (k, pt.records[k], want[k])
    assert pt.records["rec_near"].dtype == np.int64 and np.array_equal(pt.records["rec_near"], want["rec_near"])
    print("rec_min_sep", pt.records["rec_min_sep"].tolist(), "rec_near", pt.records["rec_near"].tolist(), pt.safety)
    # the records say something: an episode ended by `done` exactly where one of its minima says so (every earlier step
    # of the episode had no `done`), near misses were counted, nobody met a building
    collided = (pt.records["rec_flags"] & 4) != 0
    hit = (pt.records["rec_min_sep"] <= 0) | (pt.records["rec_min_bclear"] <= 0) | (pt.records["rec_min_wall"] < 0)
    assert collided.any() and np.array_equal(collided, hit)
    assert (pt.records["rec_near"] > 0).any() and np.isinf(pt.records["rec_min_bclear"]).all()
    assert np.isfinite(pt.records["rec_min_wall"]).all()
    assert pt.safety["episodes"] == E * quota and pt.safety["min_min_sep"] == pt.records["rec_min_sep"].min()


@pytest.mark.parametrize("fused", [True, False])
def test_safety_off_makes_no_new_launch(fused, monkeypatch):
    """safety=False: neither loop calls rvo3d_safety_scan or rvo3d_eval_account_safety, and the result is the one
    safety=True returns next to its safety figures."""
    L = _lib.lib()
    calls = {"rvo3d_safety_scan": 0, "rvo3d_eval_account_safety": 0}

    def counting(name):
        fn = getattr(L, name)

        def wrapper(*a):
            calls[name] += 1
            return fn(*a)
        return wrapper
    for name in calls:
        monkeypatch.setattr(L, name, counting(name))

    def run(safety):
        env = BatchedDroneEnv(_eval_world(), neighbors_num=5)
        pt = post_train(env, num_episodes=4, max_ep_len=12, acceler_vel=1.0, inf_print=False, fused=fused, poll_every=3,
                        safety=safety)
        res = pt.policy_test(policy_type="des_vel")
        env.close()
        return pt, res

    off, res_off = run(False)
    assert calls == {"rvo3d_safety_scan": 0, "rvo3d_eval_account_safety": 0}
    assert off.safety is None
    on, res_on = run(True)
    assert calls["rvo3d_eval_account_safety" if fused else "rvo3d_safety_scan"] > 0
    assert res_on == res_off
    assert on.safety["episodes"] == res_on["episodes"] and on.safety["near_per_1000_drone_steps"] >= 0
