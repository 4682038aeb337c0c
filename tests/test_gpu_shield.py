"""The action shield on the device (include/rvo3d.h: rvo3d_shield_action) against the plain-Python restatement
tests/shield_ref.py, which is fed the device's own pref_vel: out_vel, status, flags, slack and totals bit for bit, the
action's bits on every row that is not intervened, the command of the intervened rows to orca_ref.CONVERTER_TOL (atan2 and
asin are the device library's); pref_vel against a plain env.step of the same action on a twin env, bit for bit; and the
housekeeping: aliasing, accumulation, guard rows, the state, the shared workspace, the refusals.

Shapes (CASES): 2 x 64 with 12 buildings per env and a motion - one full wave; 2 x 70 with drone counts (70, 37) - two
waves, ghost lanes, a ghost-only wave; 1 x 8 with 70 buildings - two building tiles at T = 64; 1 x 130 - three waves.  Every
scene has two parked drones per env (dest set, no velocity) and two rows with a non-finite action.  The 3 x 4 swap scene
is flown in tests/test_gpu_shield_eval.py."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, World, _lib
from rvo3d_amd.building_motion import BuildingMotion
import building_rows_moving_ref as ref8
import shield_ref as ref

pytestmark = pytest.mark.gpu
DT = 1.0
MOVES = 3
# (E, N, buildings per env, moving, drone counts, map side, parameters, what)
PAR = dict(time_horizon=5.0, time_step=1.0, max_speed=2.0, neighbor_dist=10.0, max_neighbors=10, max_buildings=4,
           reach=10.0, below=1.0, clear_xy=0.25)
CASES = [
    (2, 64, 12, True, None, 24.0, PAR, "one full wave, 12 moving buildings"),
    (2, 70, 3, True, (70, 37), 14.0, dict(PAR, max_neighbors=16, time_horizon=3.0), "two waves, drone counts"),
    (1, 8, 70, False, None, 40.0, dict(PAR, max_neighbors=3, max_buildings=8, clear_xy=0.0), "two building tiles"),
    (1, 130, 0, False, None, 34.0, dict(PAR, max_buildings=0), "three waves"),
]
IDS = [c[-1] for c in CASES]
DIAG = ("pref_vel", "out_vel", "status", "flags", "slack")


@functools.lru_cache(maxsize=None)
def scene(E, N, nb, moving, drone_counts, side):
    """E x N drones on a side x side x 6 map with a velocity along their heading, an action of up to +-0.4 per component,
    per-env sets of nb buildings (patrolling with `moving`); rows 3 and N - 2 of every env are parked, rows 1 and N - 3
    carry a non-finite action."""
    rng = np.random.default_rng(1000 * E + N + 7 * nb)
    ms = np.array([side, side, 6.0])
    pos = rng.uniform(0.0, 1.0, (E, N, 3)) * ms
    speed, yaw, pitch = rng.uniform(0.0, 1.2, (E, N)), rng.uniform(0.0, 360.0, (E, N)), rng.uniform(-30.0, 30.0, (E, N))
    speed[:, ::9] = 0.0
    cy, sy, cp, sp = np.cos(np.radians(yaw)), np.sin(np.radians(yaw)), np.cos(np.radians(pitch)), np.sin(np.radians(pitch))
    vel = np.stack([speed * cp * cy, speed * cp * sy, speed * sp], axis=-1)
    rad = np.round(rng.uniform(0.15, 0.4, (E, N)), 3)
    dest = np.zeros((E, N), np.uint8)
    dest[:, [3, N - 2]] = 1
    vel[dest != 0] = 0.0
    action = rng.uniform(-0.4, 0.4, (E, N, 3))
    action[:, 1, 0], action[:, N - 3, 2] = np.nan, -np.inf
    wp = np.zeros((E, N, 2, 3))
    wp[:, :, 0], wp[:, :, 1] = [1.0, 1.0, 1.0], [side - 1.0, side - 1.0, 5.0]
    dc = None if drone_counts is None else np.array(drone_counts, np.int32)
    bld = np.concatenate([rng.uniform(0, side, (E, nb, 2)), rng.uniform(2, 12, (E, nb, 1)), rng.uniform(0.4, 1.5, (E, nb, 1))], axis=-1)
    sc = types.SimpleNamespace(E=E, N=N, nb=nb, pos=pos, vel=vel, yaw=yaw, pitch=pitch, rad=rad, dest=dest, action=action,
                               drone_counts=dc, bld0=bld, ends=None, speed=None)
    sc.world = World(wp, np.full((E, N), 2, np.int32), ms, bld if nb else np.zeros((0, 4)), None, dc)
    if moving:
        ends = np.zeros((E, nb, 2, 2))
        ends[:, :, 0] = bld[..., :2]
        ends[:, :, 1] = bld[..., :2] + rng.uniform(-6, 6, (E, nb, 2))
        sc.ends, sc.speed = ends, rng.uniform(0.3, 1.2, (E, nb))
        sc.speed[:, ::3] = 0.0
    return sc


def live_env(sc):
    """The env of the scene in the scene's state, its patrols attached and advanced MOVES times."""
    env = BatchedDroneEnv(sc.world, neighbors_num=3, radius=sc.rad)
    motion = None
    if sc.ends is not None:
        motion = BuildingMotion(sc.ends, sc.speed, dt=DT)
        env.attach_building_motion(motion)
        for _ in range(MOVES):
            motion.advance()
    env.set_state(pos=sc.pos, vel=sc.vel, yaw=sc.yaw, pitch=sc.pitch, dest=sc.dest)
    return env, motion


def restate(sc, motion, pref, par):
    """shield_ref.shield_env for every env, on the buildings as the device holds them -> dict of [E, N(, 3)] arrays."""
    out = {k: [] for k in ("out_action",) + DIAG + ("totals",)}
    kw = {k: v for k, v in par.items() if k != "max_speed"}
    for e in range(sc.E):
        n_live = sc.N if sc.drone_counts is None else int(sc.drone_counts[e])
        bld, vel_of = (sc.bld0[e] if sc.nb else np.zeros((0, 4))), None
        if motion is not None:
            bld, leg = motion.buildings.cpu().numpy()[e], motion.leg.cpu().numpy()[e]
            vel_of = lambda j, e=e, bld=bld, leg=leg: ref8.velocity(bld[j], sc.ends[e, j], sc.speed[e, j], leg[j], DT)[:2]
        r = ref.shield_env(sc.pos[e], sc.vel[e], sc.yaw[e], sc.pitch[e], sc.rad[e], sc.dest[e] != 0, n_live, sc.action[e],
                           bld, vel_of, pref=pref[e], max_speed=par["max_speed"], **kw)
        for k in out:
            out[k].append(r[k])
    return {k: np.stack(v) for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def cpu(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize("E,N,nb,moving,drone_counts,side,par,what", CASES, ids=IDS)
def test_device_equals_the_restatement(E, N, nb, moving, drone_counts, side, par, what):
    sc = scene(E, N, nb, moving, drone_counts, side)
    env, motion = live_env(sc)
    totals = torch.zeros((E, 4), dtype=torch.int64, device="cuda")
    action = torch.as_tensor(sc.action, device="cuda")
    out, diag = env.shield_action(action, diagnostics=True, totals=totals, **par)
    out, diag, tot = out.cpu().numpy(), cpu(diag), totals.cpu().numpy()
    want = restate(sc, motion, diag["pref_vel"], par)
    live = np.ones((E, N), bool) if drone_counts is None else np.arange(N)[None, :] < np.array(drone_counts)[:, None]
    judged = live & (sc.dest == 0) & np.isfinite(sc.action).all(axis=-1)
    intervened = (want["flags"] & ref.INTERVENED) != 0
    print(what, "judged", judged.sum(), "intervened", intervened.sum(), "totals", tot.tolist(), "status 1 / 2 / 3",
          [int((want["status"] == s).sum()) for s in (1, 2, 3)])
    assert np.array_equal(diag["status"], want["status"]) and np.array_equal(diag["flags"], want["flags"])
    assert np.array_equal(bits(diag["slack"]), bits(want["slack"]))
    assert np.array_equal(bits(diag["out_vel"]), bits(want["out_vel"]))
    assert np.array_equal(tot, want["totals"])
    assert np.array_equal(judged, want["status"] > 0)
    # S4: the action's bits where nothing was done (parked and non-finite rows among them), the command where it was
    same = live & ~intervened
    assert np.array_equal(bits(out[same]), bits(sc.action[same]))
    assert not out[~live].any()
    worst = float(np.abs(out[intervened] - want["out_action"][intervened]).max())
    print("largest |device - restatement| of a command:", worst, "tolerance", ref.CONVERTER_TOL)
    assert worst <= ref.CONVERTER_TOL
    # S5: rows that are not judged carry zeros
    for k in DIAG:
        assert not diag[k][~judged].any(), k
    floor = 1 if N == 8 else 4                                    # (of the 8 drones 4 are judged; on the CPU: 1 and 3)
    assert intervened.sum() >= floor and (judged & ~intervened).sum() >= floor
    assert np.isfinite(diag["out_vel"]).all() and np.isfinite(out[judged]).all()
    if what == "two building tiles":
        assert (want["status"][judged] >= 1).all()
    env.close()


@pytest.mark.parametrize("E,N,nb,moving,drone_counts,side,par,what", CASES, ids=IDS)
def test_pref_vel_is_the_velocity_the_step_flies(E, N, nb, moving, drone_counts, side, par, what):
    """S1 against the step itself: a plain env.step(action) on a twin env leaves env.vel bit-equal to pref_vel on every
    judged row (the rows with a non-finite action step with 0 on the twin and are not compared)."""
    sc = scene(E, N, nb, moving, drone_counts, side)
    env, _ = live_env(sc)
    twin, _ = live_env(sc)
    _, diag = env.shield_action(torch.as_tensor(sc.action, device="cuda"), diagnostics=True, **par)
    twin.step(torch.as_tensor(np.nan_to_num(sc.action, nan=0.0, posinf=0.0, neginf=0.0), device="cuda"))
    flown, pref, status = twin.vel.cpu().numpy(), diag["pref_vel"].cpu().numpy(), diag["status"].cpu().numpy()
    judged = status > 0
    assert judged.sum() >= (E * N) // 3
    differ = np.nonzero((bits(flown) != bits(pref)).any(axis=-1) & judged)
    assert len(differ[0]) == 0, (differ, flown[differ], pref[differ])
    assert not flown[sc.dest != 0].any()                          # the step parks them whatever the action
    env.close()
    twin.close()


def test_housekeeping():
    """out_action in place; totals accumulate over three calls and are not needed; the rows in front of and behind every
    output are untouched; the ten state arrays are untouched; orca_vel before and after a shield call is bit-equal."""
    E, N, nb, moving, drone_counts, side, par, _ = CASES[1]
    sc = scene(E, N, nb, moving, drone_counts, side)
    env, _ = live_env(sc)
    okw = dict(par, pref_speed=1.0)
    before, orca_before = cpu(env.get_state()), env.orca_vel(**okw).cpu().numpy()
    action = torch.as_tensor(sc.action, device="cuda")
    totals = torch.zeros((E, 4), dtype=torch.int64, device="cuda")
    out, diag = env.shield_action(action, diagnostics=True, totals=totals, **par)
    once = totals.clone()
    for _ in range(2):
        again = env.shield_action(action, totals=totals, **par)      # (no diagnostics: the null pointers)
        assert np.array_equal(bits(again.cpu().numpy()), bits(out.cpu().numpy()))
    assert torch.equal(totals, 3 * once) and int(once[:, 0].sum()) > 0
    env.shield_action(action, **par)                                 # without totals: nothing is added anywhere
    assert torch.equal(totals, 3 * once)
    # the raw entry point into guarded buffers, out_action = action
    G = 2 * N                                                        # guard rows in front and behind
    f64 = dict(dtype=torch.float64, device="cuda")
    buf = {k: torch.full(((E * N + 2 * G) * 3,), -7.0, **f64) for k in ("act", "pref_vel", "out_vel")}
    buf["slack"] = torch.full((E * N + 2 * G,), -7.0, **f64)
    buf["status"] = torch.full((E * N + 2 * G,), -7, dtype=torch.int32, device="cuda")
    buf["flags"] = torch.full((E * N + 2 * G,), 249, dtype=torch.uint8, device="cuda")
    buf["totals"] = torch.full((E * 4 + 8,), -7, dtype=torch.int64, device="cuda")
    buf["totals"][4:4 + E * 4] = 0
    buf["act"][3 * G:3 * (G + E * N)] = action.reshape(-1)
    at = lambda k, w: buf[k].data_ptr() + G * w * buf[k].element_size()
    a = _lib.ShieldArgs(*[float(par[k]) for k in ("time_horizon", "time_step", "max_speed", "neighbor_dist")],
                        par["max_neighbors"], par["max_buildings"], par["reach"], par["below"], par["clear_xy"],
                        at("act", 3), at("act", 3), at("pref_vel", 3), at("out_vel", 3), at("status", 1), at("flags", 1),
                        at("slack", 1), buf["totals"].data_ptr() + 32)
    m, dt = env._motion_args()
    assert _lib.lib().rvo3d_shield_action(env._h, C.byref(a), m, dt, env._stream()) == 0
    torch.cuda.synchronize()
    inner = lambda k, w: buf[k][G * w:(G + E * N) * w]
    assert np.array_equal(bits(inner("act", 3).cpu().numpy()), bits(out.reshape(-1).cpu().numpy()))   # in place: the same bytes
    for k, w in (("pref_vel", 3), ("out_vel", 3), ("status", 1), ("flags", 1), ("slack", 1)):
        assert torch.equal(inner(k, w), diag[k].reshape(-1)), k
    assert torch.equal(buf["totals"][4:4 + E * 4], once.reshape(-1))
    for k, w in (("act", 3), ("pref_vel", 3), ("out_vel", 3), ("status", 1), ("flags", 1), ("slack", 1)):
        guard = torch.cat([buf[k][:G * w], buf[k][(G + E * N) * w:]])
        assert (guard == (249 if k == "flags" else -7)).all(), k
    assert (buf["totals"][:4] == -7).all() and (buf["totals"][4 + E * 4:] == -7).all()
    after = cpu(env.get_state())
    assert len(before) == 10
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    assert np.array_equal(bits(env.orca_vel(**okw).cpu().numpy()), bits(orca_before))
    with pytest.raises(ValueError):
        env.shield_action(action[:, :, :2])
    with pytest.raises(ValueError):
        env.shield_action(action, totals=torch.zeros((E, 4), dtype=torch.int32, device="cuda"))
    env.close()


def raw(env, action, out, diag=None, totals=None, motion="attached", dt=DT, args=True, **kw):
    par = dict(PAR)
    par.update(kw)
    a = _lib.ShieldArgs(par["time_horizon"], par["time_step"], par["max_speed"], par["neighbor_dist"], par["max_neighbors"],
                        par["max_buildings"], par["reach"], par["below"], par["clear_xy"],
                        None if action is None else action.data_ptr(), None if out is None else out.data_ptr(),
                        *[None if diag is None else diag[n].data_ptr() for n in DIAG],
                        None if totals is None else totals.data_ptr())
    m = motion
    if isinstance(motion, str):
        m = None if env._motion is None else env._motion._args
    return _lib.lib().rvo3d_shield_action(env._h, C.byref(a) if args else None, None if m is None else C.byref(m), dt,
                                          env._stream())


def test_refused_calls_write_nothing():
    E, N, nb, moving, drone_counts, side, par, _ = CASES[0]
    sc = scene(E, N, nb, moving, drone_counts, side)
    env, motion = live_env(sc)
    f = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda")
    action, out = torch.as_tensor(sc.action, device="cuda"), f((E, N, 3), torch.float64, -7.0)
    diag = dict(pref_vel=f((E, N, 3), torch.float64, -7.0), out_vel=f((E, N, 3), torch.float64, -7.0),
                status=f((E, N), torch.int32, -7), flags=f((E, N), torch.uint8, 249), slack=f((E, N), torch.float64, -7.0))
    totals = f((E, 4), torch.int64, -7)
    inf, nan = float("inf"), float("nan")
    bad = [dict(time_horizon=0.0), dict(time_horizon=nan), dict(time_step=0.0), dict(time_step=inf), dict(max_speed=-1.0),
           dict(max_speed=nan), dict(neighbor_dist=0.0), dict(neighbor_dist=nan), dict(max_neighbors=0),
           dict(max_neighbors=17), dict(max_buildings=-1), dict(max_buildings=9), dict(reach=0.0), dict(reach=inf),
           dict(below=-1.0), dict(below=nan), dict(clear_xy=-1.0), dict(clear_xy=inf), dict(dt=-1.0), dict(dt=inf),
           dict(dt=nan), dict(args=False)]
    codes = set()
    for kw in bad:
        rc = raw(env, action, out, diag, totals, **kw)
        assert rc < 0, kw
        assert _lib.lib().rvo3d_last_error(), kw
        codes.add(rc)
    codes.add(raw(env, None, out, diag, totals))
    codes.add(raw(env, action, None, diag, totals))
    assert len(codes) == 1   # RVO3D_ERR_INVALID
    invalid = codes.pop()
    for field in ("ends", "speed", "leg"):
        m = _lib.BuildingMotionArgs(motion._args.ends, motion._args.speed, motion._args.leg)
        setattr(m, field, None)
        assert raw(env, action, out, diag, totals, motion=m) == invalid, field
    shared = scene(*CASES[3][:6])                                     # no per-env sets: a motion is refused
    env2, _ = live_env(shared)
    act2, out2 = torch.as_tensor(shared.action, device="cuda"), f((1, 130, 3), torch.float64, -7.0)
    state = raw(env2, act2, out2, motion=motion._args)
    assert state < 0 and state != invalid
    with pytest.raises(_lib.RVO3DError):
        env.shield_action(action, max_neighbors=17)
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (out2 == -7.0).all() and (totals == -7).all()
    for k, v in diag.items():
        assert (v == (249 if k == "flags" else -7)).all(), k
    assert np.array_equal(bits(action.cpu().numpy()), bits(sc.action))
    totals.zero_()
    assert raw(env, action, out, diag, totals) == 0 and raw(env2, act2, out2, motion=None) == 0   # the good calls go through
    torch.cuda.synchronize()
    assert not (out == -7.0).any() and not (out2 == -7.0).any() and (diag["status"] >= 0).all() and int(totals[:, 0].sum()) > 0
    env.close()
    env2.close()
