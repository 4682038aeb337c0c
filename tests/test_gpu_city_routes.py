"""Route re-draws in a city on the GPU (rvo3d_sample_routes_city / rvo3d_plan_routes; CityRoutePlanner,
BatchedDroneEnv.device_buildings, multi_ppo(route_sampler=planner)).

Three yardsticks.  Both kernels are compared bit for bit with their numpy restatement (CityRoutePlanner.sample_numpy /
plan_numpy), whose counts, dense check and oracle step tests/test_city_routes_host.py holds.  A re-draw is compared with
an env freshly loaded with the world the restatement gives.  And the planned routes are walked through the env's own
collision predicate: set_state along every route, one zero-action step, done stays 0 - where the straight legs raise it."""
import functools

import numpy as np
import pytest
import torch

import city_case
from city_case import DRAW, MAP, N as N_REF, planner
from rvo3d_amd import BatchedDroneEnv, synthetic_actions, synthetic_world
from test_gpu_routes import STATE_KEYS, assert_handles_equal, host, same

pytestmark = pytest.mark.gpu

NAMES = ("waypoints", "n_points", "unplaced", "blocked", "blocked_mask")
# E, N, buildings per env, P: one drone; a partial wave; a full wave; two waves with ghost lanes, at 8, 3 and 2 rows;
# P = 20 keeps a lane's points in its rows of `waypoints` (beyond 16 they leave private memory)
SHAPES = [(3, 1, 12, 8), (3, 5, 12, 8), (2, 64, 12, 8), (8, 70, 12, 8), (8, 70, 12, 3), (8, 70, 12, 2), (3, 5, 12, 20)]


def city(E, nb=12):
    return city_case.city_world(E, nb).buildings  # [E, nb, 4]: env e's set does not depend on E


@functools.lru_cache(maxsize=None)
def long_city():
    """[2, 300, 4]: env e's twelve buildings somewhere among 288 thin masts (r 0.05 .. 0.3) - past the 256 records a
    workgroup stages in LDS."""
    rng = np.random.Generator(np.random.Philox(key=77))
    b = np.round(np.stack([rng.uniform(2, 38, (2, 300)), rng.uniform(2, 38, (2, 300)), rng.uniform(3, 10, (2, 300)),
                           rng.uniform(0.05, 0.3, (2, 300))], axis=-1), 2)
    for e in range(2):
        b[e, rng.choice(300, 12, replace=False)] = city(2)[e]
    return b


def restated(E, N, P, bld, counts=None, draw=DRAW):
    pl = planner()
    wp, _, unp = pl.sample_numpy(E, N, P, draw, bld, counts)
    return (unp,) + pl.plan_numpy(wp, bld, counts)


def on_device(E, N, P, bld, counts=None, draw=DRAW, env_mask=None, out=None):
    """sample + plan: the five outputs as numpy, in NAMES' order."""
    pl = planner()
    s_out = p_out = None
    if out is not None:
        s_out, p_out = (out[0], out[1], out[2]), (out[1], out[3], out[4])
    wp, npts, unp = pl.sample(E, N, P, draw, "cuda", bld, counts, env_mask, s_out)
    assert same(host(npts), np.full((E, N), 2)) or env_mask is not None
    wp2, npts, blocked, mask = pl.plan(wp, bld, counts, env_mask, p_out)
    assert wp2 is wp
    return tuple(host(t) for t in (wp, npts, unp, blocked, mask))


def assert_same_outputs(got, want, what, rows=slice(None)):
    unp, wp, npts, blocked, mask = want
    for g, w, k in zip(got, (wp, npts, unp, blocked, mask), NAMES):
        assert g.dtype == w.dtype, k
        assert same(g[rows], w[rows]), f"{what}: {k}"


# ---- 8. both kernels equal the numpy restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize("E,N,nb,P", SHAPES)
def test_sample_and_plan_equal_the_numpy_restatement(E, N, nb, P):
    bld = city(E, nb)
    want = restated(E, N, P, bld)
    assert_same_outputs(on_device(E, N, P, bld), want, f"{E}x{N} P={P}")
    if N >= 64:  # the comparison covers detours and failures
        assert (want[2] > 2).any() or P == 2
        assert want[4].any()


def test_a_shared_list():
    bld = city(1)[0]  # [12, 4]: env_stride = 0
    want = restated(8, N_REF, 8, bld)
    assert_same_outputs(on_device(8, N_REF, 8, bld), want, "shared list")
    assert_same_outputs(on_device(8, N_REF, 8, bld[None]), want, "shared list as [1, nb, 4]")
    assert not same(want[1], restated(8, N_REF, 8, city(8))[1])


def test_counts_with_a_zero():
    counts = np.array([12, 0, 12, 5, 0, 12, 12, 1], dtype=np.int32)
    bld = city(8).copy()
    bld[3, 5:] = np.nan  # the records behind a count are not looked at
    want = restated(8, N_REF, 8, city(8), counts)
    assert_same_outputs(on_device(8, N_REF, 8, bld, counts), want, "counts")
    assert (want[2][counts == 0] == 2).all() and (want[2][counts == 12] > 2).any()
    assert_same_outputs(on_device(8, N_REF, 8, bld, torch.from_numpy(counts).cuda()), want, "counts as a device tensor")


@pytest.mark.parametrize("counts", [None, (300, 12), (257, 256)])
def test_a_list_longer_than_the_lds_cap(counts):
    """300 records per env: read from global memory - and, with counts, next to an env whose records are staged."""
    bld = long_city()
    cnt = None if counts is None else np.array(counts, dtype=np.int32)
    want = restated(2, 5, 8, bld, cnt)
    assert_same_outputs(on_device(2, 5, 8, bld, cnt), want, f"long list, counts {counts}")
    many = restated(2, 64, 8, bld, cnt)
    assert_same_outputs(on_device(2, 64, 8, bld, cnt), many, f"long list, 64 drones, counts {counts}")
    assert (many[2] > 2).any()


def test_no_buildings_on_the_device():
    pl = planner()
    plain = pl.sampler.sample(3, 5, 4, DRAW, "cuda")
    for bld in (None, np.zeros((0, 4)), np.zeros((3, 0, 4))):
        got = on_device(3, 5, 4, bld)
        assert same(got[0], host(plain[0])) and same(got[1], host(plain[1])) and same(got[2], host(plain[2]))
        assert not got[3].any() and not got[4].any()
    got = on_device(3, 5, 4, city(3), np.zeros(3, np.int32))
    assert same(got[0], host(plain[0])) and not got[3].any()


# ---- 9. masked envs ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E,N,P", [(3, 5, 8), (8, 70, 8), (3, 5, 20)])
def test_unmasked_envs_keep_their_sentinels(E, N, P):
    bld = city(E)
    want = restated(E, N, P, bld)
    mask = np.arange(E) % 2 == 1
    out = (torch.full((E, N, P, 3), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((E, N), -7, dtype=torch.int32, device="cuda"), torch.full((E,), -7, dtype=torch.int32, device="cuda"),
           torch.full((E,), -7, dtype=torch.int32, device="cuda"), torch.full((E, N), 7, dtype=torch.uint8, device="cuda"))
    got = on_device(E, N, P, bld, env_mask=mask, out=out)
    assert_same_outputs(got, want, "masked envs", mask)
    assert np.isnan(got[0][~mask]).all()
    for k in (1, 2, 3):
        assert (got[k][~mask] == -7).all(), NAMES[k]
    assert (got[4][~mask] == 7).all()
    for o, g in zip(out, got):
        assert same(host(o), g)  # written in place


# ---- 10. / 11. a re-draw equals a fresh load; the city comes from the env -------------------------------------------------

def assert_env_equals_fresh(env, fresh, steps, what):
    for x in (env, fresh):
        x.observe()
    for k in ("obs", "vo_count"):
        assert same(host(getattr(env, k)), host(getattr(fresh, k))), f"{what}: {k}"
    se, sf = env.get_state(), fresh.get_state()
    for k in STATE_KEYS:
        assert same(host(se[k]), host(sf[k])), f"{what}: state {k}"
    for t in range(steps):
        a = torch.from_numpy(synthetic_actions(env.E, env.N, t, 1234)).cuda()
        env.step(a, autoreset=True); fresh.step(a, autoreset=True)
        assert_handles_equal(env, fresh, np.arange(env.E), f"{what}: step {t}")
    for r, f in zip(env.routes(), fresh.routes()):
        assert same(host(r), host(f)), f"{what}: routes()"


def test_redraw_equals_a_fresh_load():
    E, N, P = 8, N_REF, 8
    w = city_case.city_world()
    pl = planner()
    env = BatchedDroneEnv(w.with_max_points(P))
    env.observe()
    for t in range(3):
        env.step(torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda(), autoreset=True)
    ret = pl.redraw(env, DRAW)
    assert len(ret) == 4
    want = restated(E, N, P, w.buildings)
    got = tuple(host(t) for t in ret) + (host(pl.last_blocked_mask),)
    assert_same_outputs((got[0], got[1], got[2], got[3], got[4]), want, "what redraw returns")
    fresh = BatchedDroneEnv(pl.world(E, N, DRAW, P, w.buildings))
    assert_env_equals_fresh(env, fresh, 6, "after redraw")
    assert env.error_flags() & 4 == 0
    # a second call reuses the staging tensors; a masked one leaves the other envs alone
    before = tuple(host(r) for r in env.routes())
    mask = np.arange(E) % 2 == 0
    again = pl.redraw(env, 2, mask)
    assert all(a is b for a, b in zip(again, ret))
    want2 = restated(E, N, P, w.buildings, draw=2)
    wp, npts = (host(r) for r in env.routes())
    assert same(wp[mask], want2[1][mask]) and same(npts[mask], want2[2][mask])
    assert same(wp[~mask], before[0][~mask]) and same(npts[~mask], before[1][~mask])
    env.close(); fresh.close()


def test_device_buildings_and_a_redraw_after_new_cities():
    E, N, P = 8, N_REF, 8
    w = city_case.city_world()
    new = synthetic_world(E, N, MAP, nb=9, per_env_buildings=True, seed=9).buildings
    counts = np.array([9, 9, 4, 9, 0, 9, 9, 9], dtype=np.int32)
    pl = planner()
    env = BatchedDroneEnv(w.with_max_points(P))
    b, c = env.device_buildings()
    assert b.dtype == torch.float64 and b.device == env.device and c is None and same(host(b), w.buildings)
    assert env.device_buildings()[0] is b  # cached
    env.set_env_buildings(new, counts)
    b2, c2 = env.device_buildings()
    assert b2 is not b and same(host(b2), new) and c2.dtype == torch.int32 and same(host(c2), counts)
    pl.redraw(env, 3)
    fresh = BatchedDroneEnv(pl.world(E, N, 3, P, new, counts))
    assert_env_equals_fresh(env, fresh, 4, "after new cities")
    old = pl.world(E, N, 3, P, w.buildings)
    assert not same(host(env.routes()[0]), old.waypoints), "the routes must go round the new city"
    env.set_env_buildings(None)  # a world of per-env sets has no shared list to go back to
    b3, c3 = env.device_buildings()
    assert tuple(b3.shape) == (1, 0, 4) and c3 is None
    pl.redraw(env, 3)
    assert same(host(env.routes()[0]), pl.sampler.sample_numpy(E, N, P, 3)[0])
    env.close(); fresh.close()
    shared = synthetic_world(4, 6, MAP, nb=5, seed=5)
    env = BatchedDroneEnv(shared)
    b, c = env.device_buildings()
    assert tuple(b.shape) == (1, 5, 4) and c is None and same(host(b)[0], shared.buildings)
    env.close()


# ---- 12. the env's own collision predicate along the planned routes --------------------------------------------------------

def along(wp, npts, s):
    """The point at share s of the arc length of each route: wp [E, 1, P, 3], npts [E, 1] -> [E, 1, 3]."""
    out = np.empty((wp.shape[0], 1, 3))
    for e in range(wp.shape[0]):
        r = wp[e, 0, :npts[e, 0]]
        seg = np.linalg.norm(np.diff(r, axis=0), axis=1)
        cum = np.concatenate([[0.0], np.cumsum(seg)])
        t = s * cum[-1]
        k = min(int(np.searchsorted(cum, t, side="right")) - 1, len(seg) - 1)
        out[e, 0] = r[k] + (t - cum[k]) / seg[k] * (r[k + 1] - r[k])
    return out


def test_the_env_meets_no_building_along_the_planned_routes():
    """256 envs of one drone (nobody else to collide with) in one shared city of 12 buildings.  Failed routes stand
    still at their start (which is clear)."""
    E, P, K = 256, 8, 64
    w = synthetic_world(E, 1, MAP, nb=12, seed=5)
    pl = planner()
    env = BatchedDroneEnv(w.with_max_points(P))
    wp, npts, unp, blocked = (host(t) for t in pl.redraw(env, DRAW))
    failed = host(pl.last_blocked_mask).astype(bool)
    assert int(unp.sum()) == 0 and failed.sum() <= 0.05 * E and (npts > 2).sum() >= 0.15 * E
    straight = np.concatenate([wp[:, :, :1], np.take_along_axis(wp, (npts.astype(np.int64) - 1)[:, :, None, None], 2)], 2)
    two = np.full((E, 1), 2)
    zero = torch.zeros((E, 1, 3), dtype=torch.float64, device="cuda")

    def walk(rows, counts):
        env.reset()
        hits = np.zeros((E, 1), dtype=bool)
        for s in np.linspace(0.0, 1.0, K):
            pos = along(rows, counts, s)
            pos[failed] = rows[failed][:, 0]
            env.set_state(pos=pos)
            hits |= host(env.step(zero)[3]) != 0
        return hits

    assert walk(straight, two).sum() > 0, "the straight legs must meet buildings, or this proves nothing"
    assert walk(wp, npts).sum() == 0
    env.close()


# ---- 13. the trainer -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [True, False])
def test_trainer_redraws_round_the_city(fused):
    """mlp_ac, 16 drones x 8 envs in their own cities, 6 steps per epoch, two collect() calls with the planner as
    route_sampler and redraw_every = 1: after each collect the routes are the restatement's for draw = epoch and the next
    epoch starts from observe() of a fresh env over planner.world(draw = epoch), bit for bit."""
    from rvo3d_amd.policy import mlp_ac, multi_ppo
    N, E, P, steps = 16, 8, 6, 6
    w = synthetic_world(E, N, MAP, min_sep=0.8, nb=12, per_env_buildings=True, seed=5)
    pl = planner()
    env = BatchedDroneEnv(w.with_max_points(P))
    torch.manual_seed(0)
    ac = mlp_ac(env.W).cuda()
    tr = multi_ppo(env, ac, steps_per_epoch=steps, max_ep_len=9, train_pi_iters=1, train_v_iters=1, seed=3,
                   fused_rollout=fused, route_sampler=pl, redraw_every=1)
    assert bool(tr._fused_ok()) == fused
    env.reset(); env.observe()
    for epoch in range(2):
        tr.buf.ptr = 0
        tr.collect()
        want = pl.world(E, N, epoch, P, w.buildings)
        assert (want.n_points > 2).any()
        wp, npts = env.routes()
        assert same(host(wp), want.waypoints) and same(host(npts), want.n_points), f"routes after epoch {epoch}"
        fresh = BatchedDroneEnv(want)
        fo, fc = fresh.observe()
        assert same(host(tr._cur[0]), host(fo)) and same(host(tr._cur[1]), host(fc)), f"next epoch's start, epoch {epoch}"
        fs, es = fresh.get_state(), env.get_state()
        for k in STATE_KEYS:
            assert same(host(es[k]), host(fs[k])), k
        fresh.close()
    env.close()
