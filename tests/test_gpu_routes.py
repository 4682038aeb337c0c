"""Routes re-drawn on the device (rvo3d_set_routes / rvo3d_get_routes / rvo3d_sample_routes; BatchedDroneEnv.set_routes,
RouteSampler, multi_ppo(route_sampler=...)) on the GPU.

Two yardsticks.  The sampler kernel is compared bit for bit with its numpy restatement (RouteSampler.sample_numpy, whose
counts tests/test_routes_host.py pins).  set_routes is compared with rvo3d_load_world, which test_gpu_parity.py pins to the
reference: an env that took new routes must behave bit for bit as the env of a handle freshly loaded with them, an env
that did not as if nothing had been called.

Inputs of the set_routes comparison: map (24, 24, 8), P = 3, n_points 3 for even drones and 2 for odd ones (their third
row is padding), W1 = synthetic_world(seed=41, n_points=3), W2 = seed 43.  Handle A loads W1 and takes 7 auto-reset steps
of synthetic_actions, then set_routes(W2) on the envs with e % 2 == 0 and observe; handle C is freshly loaded with W2,
handle D with W1 (it takes the 7 steps and every later call but set_routes).  Three drivers for the steps after the call:

  synthetic  25 steps of synthetic_actions(t = 7 .. 31), the same tensors for the three handles.
  des_vel    25 steps, each handle fed its own des_vel() as float64 actions (uaisa_env/gym_env_test.py:12 does that).  The
             env reads an action as (acceleration, yaw rate, pitch rate), so these drones circle and leave the map: on the
             CPU oracle NO drone of W2 passes waypoint 1 or finishes within 400 such steps (wp_idx > 1: 0, finish: 0, for
             all five shapes).  Kept as a second set of actions that depend on each handle's own state.
  follow     40 steps, each handle fed a steering of its own des_vel(): yaw / pitch towards it, speed towards 0.5 (0.5 m
             per step against the 0.4 m arrival radius).  These drones switch waypoints and arrive, so route lengths
             (extra_len = real_len - route_len at the destination) and the padded waypoint are exercised.  On the CPU
             oracle, W2's even envs, first step with wp_idx > 1 / first finish / finishes within 40 steps / drones with
             extra_len != 0 after 40 steps:
                 8 x 21    5 / 10 /  88 /  58        16 x 13   2 / 10 / 104 /  70      48 x 6   4 / 8 / 121 / 84
                 64 x 6    4 /  4 / 184 / 108        100 x 3   4 /  4 / 181 / 108
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, RouteSampler, World, _lib, synthetic_actions, synthetic_world

pytestmark = pytest.mark.gpu

MAP = (24.0, 24.0, 8.0)
SHAPES = [(8, 21), (16, 13), (48, 6), (64, 6), (100, 3)]  # several envs per wave + a partial last workgroup (x2);
#                                                             padded kernel with ghost lanes; exact 64; two waves
OUT_KEYS = ("obs", "vo_count", "reward", "done", "info", "finish", "reset_mask")
STATE_KEYS = ("pos", "vel", "yaw", "pitch", "real_len", "max_dev", "extra_len", "wp_idx", "arrive", "dest")
# the sampler's cases (tests/test_routes_host.py pins their counts): envs, drones, map, min_sep, min_len, max_tries
SAMPLER_CASES = [(5, 8, (20.0, 20.0, 8.0), 3.0, 8.0, 32), (3, 64, (20.0, 20.0, 8.0), 2.0, 6.0, 32),
                 (2, 100, (24.0, 24.0, 8.0), 1.5, 6.0, 32), (2, 256, (40.0, 40.0, 10.0), 1.5, 10.0, 32),
                 (3, 64, (20.0, 20.0, 8.0), 2.0, 6.0, 4)]


def host(t):
    return t.cpu().numpy()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_envs_equal(a, b, envs, what):
    """Two arrays' rows `envs` bit for bit, NaN == NaN for floats: no tolerance."""
    assert same(host(a)[envs], host(b)[envs]), what


def assert_handles_equal(a, b, envs, what):
    for k in OUT_KEYS:
        assert_envs_equal(getattr(a, k), getattr(b, k), envs, f"{what}: {k}")
    sa, sb = a.get_state(), b.get_state()
    for k in STATE_KEYS:
        assert_envs_equal(sa[k], sb[k], envs, f"{what}: state {k}")


@functools.lru_cache(maxsize=None)
def worlds(N, E):
    """(W1, W2): three-row routes of which the odd drones use two."""
    npts = np.repeat(np.where(np.arange(N) % 2 == 0, 3, 2)[None], E, 0).astype(np.int32)
    out = []
    for seed in (41, 43):
        w = synthetic_world(E, N, MAP, n_points=3, seed=seed)
        out.append(World(w.waypoints, npts.copy(), w.map_size))
    return tuple(out)


def padded(w):
    """A world's waypoints as the handle stores them: rows behind n_points hold the destination."""
    wp = np.array(w.waypoints, dtype=np.float64)
    E, N, P, _ = wp.shape
    last = np.take_along_axis(wp, (w.n_points.astype(np.int64) - 1)[:, :, None, None], axis=2)
    fill = np.arange(P)[None, None, :, None] >= w.n_points[:, :, None, None]
    return np.where(fill, last, wp)


def follow(env):
    """Steer towards the env's own des_vel(): (speed towards 0.5, yaw rate, pitch rate), 2 decimals, float64."""
    dv, st = env.des_vel(), env.get_state()
    want_yaw = torch.rad2deg(torch.atan2(dv[..., 1], dv[..., 0]))
    want_pit = torch.rad2deg(torch.atan2(dv[..., 2], torch.hypot(dv[..., 0], dv[..., 1])))
    moving = (dv != 0).any(-1)
    dy = torch.where(moving, torch.remainder(want_yaw - st["yaw"] + 180.0, 360.0) - 180.0, 0.0)
    dp = torch.where(moving, want_pit - st["pitch"], 0.0)
    acc = 0.5 - torch.linalg.vector_norm(st["vel"], dim=-1)
    a = torch.stack([acc, dy / 90.0, dp / 90.0], dim=-1).clamp(-1.0, 1.0)
    return torch.round(a * 100.0) / 100.0


@functools.lru_cache(maxsize=None)
def run_set_routes(N, E, driver):
    """Handles A, C, D of the module docstring, compared after every step; returns the tallies the tests assert on."""
    w1, w2 = worlds(N, E)
    A, Cn, D = BatchedDroneEnv(w1), BatchedDroneEnv(w2), BatchedDroneEnv(w1)
    masked, unmasked = np.arange(0, E, 2), np.arange(1, E, 2)
    mask = np.arange(E) % 2 == 0
    for x in (A, D):
        x.observe()
        for t in range(7):
            x.step(torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda(), autoreset=True)
    assert_handles_equal(A, D, np.arange(E), "before the call")
    # numpy in one driver, device tensors (bool mask) in the others
    if driver == "synthetic":
        A.set_routes(w2.waypoints, w2.n_points, mask)
    else:
        A.set_routes(torch.from_numpy(w2.waypoints).cuda(), torch.from_numpy(w2.n_points).cuda(),
                     torch.from_numpy(mask).cuda())
    for x in (A, Cn, D):
        x.observe()
    tally = dict(first_obs_differs=not same(host(A.obs)[masked], host(D.obs)[masked]), wp_gt1=0, finish=0, done=0,
                 extra_len=0)
    for k in ("obs", "vo_count"):
        assert_envs_equal(getattr(A, k), getattr(Cn, k), masked, f"observe after the call: {k}")
        assert_envs_equal(getattr(A, k), getattr(D, k), unmasked, f"observe after the call, unmasked: {k}")
    sa, sc, sd = A.get_state(), Cn.get_state(), D.get_state()
    for k in STATE_KEYS:
        assert_envs_equal(sa[k], sc[k], masked, f"state after the call: {k}")
        assert_envs_equal(sa[k], sd[k], unmasked, f"state after the call, unmasked: {k}")
    steps = 40 if driver == "follow" else 25
    for t in range(7, 7 + steps):
        if driver == "synthetic":
            acts = [torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()] * 3
        elif driver == "des_vel":
            acts = [x.des_vel() for x in (A, Cn, D)]
        else:
            acts = [follow(x) for x in (A, Cn, D)]
        for x, a in zip((A, Cn, D), acts):
            assert a.dtype == torch.float64
            x.step(a, autoreset=True)
        assert_handles_equal(A, Cn, masked, f"{N}x{E} {driver} step {t}, masked envs against the fresh handle")
        assert_handles_equal(A, D, unmasked, f"{N}x{E} {driver} step {t}, unmasked envs against the untouched handle")
        tally["wp_gt1"] += int((host(A.get_state()["wp_idx"])[masked] > 1).sum())
        tally["finish"] += int(host(A.finish)[masked].sum())
        tally["done"] += int(host(A.done)[masked].sum())
    tally["extra_len"] = int((host(A.get_state()["extra_len"])[masked] != 0).sum())
    ra, rc, rd = A.routes(), Cn.routes(), D.routes()
    for i, k in enumerate(("waypoints", "n_points")):
        assert_envs_equal(ra[i], rc[i], masked, f"routes(): {k}")
        assert_envs_equal(ra[i], rd[i], unmasked, f"routes(), unmasked: {k}")
    mix = np.where(mask[:, None, None, None], padded(w2), padded(w1))
    assert same(host(ra[0]), mix), "routes() is the mixture of W1 and W2, padded with each destination"
    assert same(host(ra[1]), w1.n_points)  # (the same counts in both worlds)
    assert A.error_flags() & 4 == 0
    for x in (A, Cn, D):
        x.close()
    print(f"{N}x{E} {driver}: {tally}")
    return tally


# ---- 1. the sampler equals its restatement --------------------------------------------------------------------------------

def sampler_of(case, **kw):
    _, _, size, sep, length, tries = case
    return RouteSampler(size, min_sep=sep, min_len=length, margin=1.0, max_tries=tries, seed=41, **kw)


@functools.lru_cache(maxsize=None)
def restated(i, P=3):
    case = SAMPLER_CASES[i]
    return sampler_of(case).sample_numpy(case[0], case[1], P, 1)


@pytest.mark.parametrize("i", range(len(SAMPLER_CASES)))
def test_sampler_equals_the_numpy_restatement(i):
    case = SAMPLER_CASES[i]
    E, N = case[:2]
    want = restated(i)
    got = sampler_of(case).sample(E, N, 3, 1, "cuda")
    for g, w, k in zip(got, want, ("waypoints", "n_points", "unplaced")):
        assert g.dtype == {np.dtype("float64"): torch.float64, np.dtype("int32"): torch.int32}[w.dtype]
        assert same(host(g), w), k
    if case[5] == 4:
        assert int(want[2].sum()) == 34  # the rounds ran out: the last candidates are part of the comparison


@pytest.mark.parametrize("i", [0, 2])
def test_sampler_leaves_unmasked_rows_alone(i):
    case = SAMPLER_CASES[i]
    E, N = case[:2]
    want = restated(i)
    mask = np.arange(E) % 2 == 1
    out = (torch.full((E, N, 3, 3), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((E, N), -7, dtype=torch.int32, device="cuda"), torch.full((E,), -7, dtype=torch.int32, device="cuda"))
    got = sampler_of(case).sample(E, N, 3, 1, "cuda", env_mask=mask, out=out)
    assert all(g is o for g, o in zip(got, out))
    for g, w in zip(got, want):
        assert same(host(g)[mask], w[mask])
    assert np.isnan(host(got[0])[~mask]).all()
    assert (host(got[1])[~mask] == -7).all() and (host(got[2])[~mask] == -7).all()


def test_sampler_env_offset_on_the_device():
    """env_offset = 3, E = 2 is envs 3 and 4 of E = 5: a shard holds the routes of the whole batch."""
    case = SAMPLER_CASES[0]
    whole = sampler_of(case).sample(5, 8, 2, 1, "cuda")
    part = sampler_of(case, env_offset=3).sample(2, 8, 2, 1, "cuda")
    for w, p in zip(whole, part):
        assert same(host(w)[3:5], host(p))
    assert not same(host(whole[0])[:2], host(part[0]))


# ---- 2. / 3. set_routes equals a fresh load --------------------------------------------------------------------------------

@pytest.mark.parametrize("N,E", SHAPES)
def test_set_routes_equals_a_fresh_load(N, E):
    """Masked envs against handle C (freshly loaded with W2), unmasked envs against handle D (W1, no set_routes): obs,
    vo_count, reward, done, info, finish, reset_mask, the ten state fields after every one of 25 steps, and routes()."""
    tally = run_set_routes(N, E, "synthetic")
    assert tally["first_obs_differs"], "the new routes must show in the first observation"
    assert tally["done"] > 0, tally


@pytest.mark.parametrize("N,E", SHAPES)
def test_set_routes_equals_a_fresh_load_under_des_vel_actions(N, E):
    """Each handle driven by its own des_vel() as float64 actions (see the module docstring: these drones do not arrive)."""
    tally = run_set_routes(N, E, "des_vel")
    assert tally["first_obs_differs"] and tally["done"] > 0, tally


@pytest.mark.parametrize("N,E", SHAPES)
def test_set_routes_equals_a_fresh_load_while_drones_arrive(N, E):
    """Each handle steered along its own des_vel() for 40 steps: drones pass waypoint 1 and finish (counts of the CPU
    oracle in the module docstring), so the route lengths (extra_len) and the padded waypoint take part."""
    tally = run_set_routes(N, E, "follow")
    assert tally["first_obs_differs"], tally
    assert tally["wp_gt1"] > 0 and tally["finish"] > 0 and tally["extra_len"] > 0, tally


def test_routes_after_the_constructor():
    for N, E in ((8, 21), (100, 3)):
        w1, _ = worlds(N, E)
        env = BatchedDroneEnv(w1)
        wp, npts = env.routes()
        assert wp.dtype == torch.float64 and npts.dtype == torch.int32
        assert same(host(wp), padded(w1)) and same(host(npts), w1.n_points)
        assert not same(padded(w1), w1.waypoints)  # (there is padding to get right)
        env.close()


def test_n_points_none_means_every_row():
    N, E = 16, 13
    w1, w2 = worlds(N, E)
    full = World(w2.waypoints, np.full((E, N), 3, np.int32), w2.map_size)
    a, c = BatchedDroneEnv(w1), BatchedDroneEnv(full)
    a.set_routes(w2.waypoints)
    a.observe(); c.observe()
    for t in range(3):
        act = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        a.step(act, autoreset=True); c.step(act, autoreset=True)
        assert_handles_equal(a, c, np.arange(E), f"step {t}")
    a.close(); c.close()


# ---- 4. bad n_points -----------------------------------------------------------------------------------------------------

def test_bad_n_points_leave_their_env_alone_and_raise_the_flag():
    N, E = 16, 13
    w1, w2 = worlds(N, E)
    A, ctl, Cn = BatchedDroneEnv(w1), BatchedDroneEnv(w1), BatchedDroneEnv(w2)
    for x in (A, ctl):
        x.observe()
        for t in range(3):
            x.step(torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda(), autoreset=True)
    bad = w2.n_points.copy()
    bad[2, 5] = 1            # below 2
    bad[4, N - 1] = 3 + 1    # above max_points
    bad[3, 0] = 0            # an unmasked env: not even read
    mask = np.arange(E) % 2 == 0
    A.set_routes(w2.waypoints, bad, mask)
    assert A.error_flags() & 4
    assert A.error_flags() == 0  # read and cleared
    for x in (A, ctl, Cn):
        x.observe()
    kept = np.array([2, 4] + list(range(1, E, 2)))
    took = np.array([0, 6, 8, 10, 12])
    assert_envs_equal(A.obs, ctl.obs, kept, "refused envs: first observation")
    assert_envs_equal(A.obs, Cn.obs, took, "the other masked envs: first observation")
    for t in range(3, 8):
        act = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        for x in (A, ctl, Cn):
            x.step(act, autoreset=True)
        assert_handles_equal(A, ctl, kept, f"refused and unmasked envs, step {t}")
        assert_handles_equal(A, Cn, took, f"the other masked envs, step {t}")
    wp, npts = A.routes()
    mix = np.where(np.isin(np.arange(E), took)[:, None, None, None], padded(w2), padded(w1))
    assert same(host(wp), mix) and same(host(npts), w1.n_points)
    A.set_routes(w2.waypoints, bad, mask)
    with pytest.raises(ValueError, match="n_points"):
        A.check_finite()
    A.check_finite()  # cleared
    for x in (A, ctl, Cn):
        x.close()


# ---- 5. the calls' contract -------------------------------------------------------------------------------------------------

def ptr(t):
    return C.c_void_p(t.data_ptr())


def test_contract_of_set_routes_and_get_routes():
    N, E = 16, 13
    w1, w2 = worlds(N, E)
    L = _lib.lib()
    wp = torch.from_numpy(w2.waypoints).cuda()
    npts = torch.from_numpy(w2.n_points).cuda()
    # a handle without a loaded world
    cfg = _lib.Config(E, N, 3, 0, 10, 1, 0, -1, (C.c_double * 3)(*MAP))
    h = C.c_void_p()
    _lib.check(L.rvo3d_create(C.byref(cfg), C.byref(h)), "rvo3d_create")
    assert L.rvo3d_set_routes(h, None, ptr(wp), ptr(npts), None) == -3  # RVO3D_ERR_STATE
    assert b"rvo3d_load_world" in L.rvo3d_last_error()
    assert L.rvo3d_get_routes(h, ptr(wp), ptr(npts), None) == -3
    L.rvo3d_destroy(h)
    a, twin = BatchedDroneEnv(w1), BatchedDroneEnv(w1)
    for x in (a, twin):
        x.observe()
        x.step(torch.from_numpy(synthetic_actions(E, N, 0, 1234)).cuda(), autoreset=True)
    assert L.rvo3d_set_routes(a._h, None, None, ptr(npts), None) == -1  # RVO3D_ERR_INVALID
    assert b"waypoints" in L.rvo3d_last_error()
    assert L.rvo3d_set_routes(a._h, None, ptr(wp), None, None) == -1
    assert b"n_points" in L.rvo3d_last_error()
    assert L.rvo3d_set_routes(None, None, ptr(wp), ptr(npts), None) == -1
    with pytest.raises(AssertionError):
        a.set_routes(w2.waypoints[:, :, :2])
    with pytest.raises(AssertionError):
        a.set_routes(w2.waypoints, w2.n_points, np.ones(E + 1, bool))
    # either output of get_routes may be missing
    assert L.rvo3d_get_routes(a._h, None, None, None) == 0
    only = torch.zeros_like(npts)
    assert L.rvo3d_get_routes(a._h, None, ptr(only), None) == 0
    assert same(host(only), w1.n_points)
    for t in range(1, 6):
        act = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        a.step(act, autoreset=True); twin.step(act, autoreset=True)
        assert_handles_equal(a, twin, np.arange(E), f"after refused calls, step {t}")
    a.close(); twin.close()


def test_contract_of_sample_routes():
    L = _lib.lib()
    wp = torch.full((2, 8, 2, 3), float("nan"), dtype=torch.float64, device="cuda")
    npts = torch.full((2, 8), -7, dtype=torch.int32, device="cuda")
    good = RouteSampler((20.0, 20.0, 8.0))

    def call(cfg, N=8, P=2, w=wp, n=npts):
        return L.rvo3d_sample_routes(C.byref(cfg), 2, N, P, 1, None, None if w is None else ptr(w),
                                     None if n is None else ptr(n), None, None)

    cfg = good.config()
    cfg.max_tries = 0
    assert call(cfg) == -1 and b"max_tries" in L.rvo3d_last_error()
    cfg = good.config()
    cfg.lo[2] = cfg.hi[2]
    assert call(cfg) == -1 and b"lo / hi" in L.rvo3d_last_error()
    cfg.lo[2] = cfg.hi[2] + 1.0
    assert call(cfg) == -1
    cfg = good.config()
    assert call(cfg, N=513) == -1 and b"num_drones" in L.rvo3d_last_error()
    assert call(cfg, P=1) == -1
    assert call(cfg, w=None) == -1 and b"waypoints" in L.rvo3d_last_error()
    assert call(cfg, n=None) == -1 and b"n_points" in L.rvo3d_last_error()
    torch.cuda.synchronize()
    assert np.isnan(host(wp)).all() and (host(npts) == -7).all()  # refused: nothing was written
    assert call(cfg) == 0  # unplaced is optional
    assert same(host(wp), good.sample_numpy(2, 8, 2, 1)[0])


# ---- 6. checkpoint ---------------------------------------------------------------------------------------------------------

def test_checkpoint_carries_the_routes():
    N, E = 16, 13
    w1, w2 = worlds(N, E)
    a = BatchedDroneEnv(w1)
    a.observe()
    plain = set(a.state_dict())
    assert plain == set(STATE_KEYS) | {"shape"}  # an untouched env keeps today's keys
    for t in range(4):
        a.step(torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda(), autoreset=True)
    a.set_routes(w2.waypoints, w2.n_points, np.arange(E) % 2 == 0)
    a.observe()
    for t in range(4, 7):
        a.step(torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda(), autoreset=True)
    sd = a.state_dict()
    assert set(sd) == plain | {"waypoints", "n_points"}
    b = BatchedDroneEnv(w1)  # the ORIGINAL world
    b.load_state_dict(sd)
    for i, r in enumerate(b.routes()):
        assert same(host(r), host(a.routes()[i]))
    for t in range(7, 12):
        act = torch.from_numpy(synthetic_actions(E, N, t, 1234)).cuda()
        a.step(act, autoreset=True); b.step(act, autoreset=True)
        assert_handles_equal(a, b, np.arange(E), f"resumed, step {t}")
    a.close(); b.close()


# ---- 7. the trainer ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [True, False])
def test_trainer_redraws_at_the_epoch_end(fused):
    """mlp_ac, 16 drones x 8 envs, 6 steps per epoch, two collect() calls with a sampler and redraw_every = 1: after each
    collect the routes are sample_numpy(draw = epoch) and the observation the next epoch starts from is observe() of a
    fresh env over sampler.world(draw = epoch), bit for bit."""
    from rvo3d_amd.policy import mlp_ac, multi_ppo
    N, E, steps = 16, 8, 6
    w = synthetic_world(E, N, MAP, min_sep=0.8, seed=41)
    sampler = RouteSampler(MAP, min_sep=1.5, min_len=6.0, seed=41)
    env = BatchedDroneEnv(w)
    torch.manual_seed(0)
    ac = mlp_ac(env.W).cuda()
    tr = multi_ppo(env, ac, steps_per_epoch=steps, max_ep_len=9, train_pi_iters=1, train_v_iters=1, seed=3,
                   fused_rollout=fused, route_sampler=sampler, redraw_every=1)
    assert bool(tr._fused_ok()) == fused
    env.reset(); env.observe()
    for epoch in range(2):
        tr.buf.ptr = 0
        tr.collect()
        want_wp, want_n, unplaced = sampler.sample_numpy(E, N, env.P, epoch)
        assert int(unplaced.sum()) == 0
        wp, npts = env.routes()
        assert same(host(wp), want_wp) and same(host(npts), want_n), f"routes after epoch {epoch}"
        fresh = BatchedDroneEnv(sampler.world(E, N, epoch, P=env.P))
        fo, fc = fresh.observe()
        assert same(host(tr._cur[0]), host(fo)) and same(host(tr._cur[1]), host(fc)), f"next epoch's start, epoch {epoch}"
        fs, es = fresh.get_state(), env.get_state()
        for k in STATE_KEYS:  # (extra_len included: a reset keeps it, new routes zero it)
            assert same(host(es[k]), host(fs[k])), k
        fresh.close()
    assert not same(sampler.sample_numpy(E, N, env.P, 0)[0], sampler.sample_numpy(E, N, env.P, 1)[0])
    env.close()


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_without_a_sampler_keeps_the_world(fused):
    from rvo3d_amd.policy import mlp_ac, multi_ppo
    N, E, steps = 16, 8, 6
    w = synthetic_world(E, N, MAP, min_sep=0.8, seed=41)
    env = BatchedDroneEnv(w)
    torch.manual_seed(0)
    ac = mlp_ac(env.W).cuda()
    tr = multi_ppo(env, ac, steps_per_epoch=steps, max_ep_len=9, train_pi_iters=1, train_v_iters=1, seed=3,
                   fused_rollout=fused)
    env.reset(); env.observe()
    for epoch in range(2):
        tr.buf.ptr = 0
        tr.collect()
        wp, npts = env.routes()
        assert same(host(wp), w.waypoints) and same(host(npts), w.n_points)
    env.close()
