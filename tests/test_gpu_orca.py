"""The ORCA velocity and the velocity command on the device (include/rvo3d.h: rvo3d_orca_vel, rvo3d_vel_command) against
the plain-Python restatement (tests/orca_ref.py): out_vel, n_neighbors, n_buildings, status and slack bit for bit and
without exemptions, the restatement evaluated on the device's own state, env.des_vel() and the buildings as the device
holds them; the converter to the tolerance tests/test_orca_host.py measured, its clipped bits exactly; the refusals.

Shapes (CASES; the scenes, their patrols and the live buildings are those of tests/test_gpu_rvo_city.py): N 5 / 64 / 65 /
130 - part of a wave, a full wave, the wave seam, three waves; E 3..6; max_neighbors 3 (most drones have more in range), 10
and 16; nb_max 0 (the empty shared list), 1, 3 and T + 1 = 129 at N = 65 (two building tiles); per-env sets with unequal
counts, one of them 0; the shared list; counted handles with ghost rows and an env of one drone; patrols with standing,
arriving and cruising records, advanced three times; max_buildings 0, 4 and 8.  From N = 64 on the last 40 drones of
every env stand in a ball of 0.5 m: they overlap, and the planes of most have no common point.

Status counts of "three waves" (the restatement on the CPU, des_vel taken as the unit vector to the waypoint and the patrols
before their first move: tests/test_orca_host.py::test_status_counts_of_the_device_scene): status 1 / 2 / 3 = 12 / 318 / 60,
status 3 at a lane >= 64: 59.  The device test asserts half of each as a floor (STATUS_FLOORS), on the restatement of the
device's own state."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, World, _lib
import building_rows_moving_ref as ref8
import orca_ref as ref
import test_gpu_rvo_city as city

pytestmark = pytest.mark.gpu
DT = city.DT
# (E, N, nb_max, max_neighbors, max_buildings, drone counts, what): nb_max None - the shared list of 3, 0 - the empty one
CASES = [
    (3, 5, 3, 16, 8, None, "part of a wave"),
    (4, 64, 1, 3, 4, None, "a full wave, one record, three neighbours kept"),
    (3, 65, 129, 10, 8, None, "the wave seam, two tiles"),
    (3, 130, 3, 16, 4, None, "three waves"),
    (5, 64, 3, 10, 0, (64, 1, 30, 64, 7), "a counted handle, no building kept"),
    (6, 65, 3, 3, 8, (65, 64, 1, 33, 65, 2), "counted across the seam"),
    (3, 64, None, 10, 4, None, "the shared list"),
    (4, 5, 0, 10, 4, None, "no buildings at all"),
]
IDS = [c[-1] for c in CASES]
PAR = dict(time_horizon=5.0, time_step=1.0, max_speed=2.0, pref_speed=1.0, neighbor_dist=10.0, reach=10.0, below=1.0,
           clear_xy=0.25)
STATUS_FLOORS = {"three waves": (6, 159, 30, 29)}   # status 1, 2, 3, and 3 at a lane >= 64


@functools.lru_cache(maxsize=None)
def scene(E, N, nb_max, drone_counts=None):
    """test_gpu_rvo_city's scene with, from N = 64 on, the last 40 drones of every env in a ball of 0.5 m round (6, 6, 4)."""
    base = city.scene(E, N, nb_max, drone_counts)
    sc = types.SimpleNamespace(**vars(base))
    if N >= 64:
        rng = np.random.default_rng(N + 17)
        c = rng.normal(size=(E, 40, 3))
        sc.pos = base.pos.copy()
        sc.pos[:, N - 40:] = [6.0, 6.0, 4.0] + 0.5 * c / np.linalg.norm(c, axis=-1, keepdims=True) * rng.uniform(0, 1, (E, 40, 1)) ** (1 / 3)
        sc.vel = base.vel.copy()
        sc.vel[:, N - 40:] *= 0.3
    return sc


def restate(sc, des, bld, mot, **kw):
    """orca_ref.orca_env for every env of the scene -> dict of [E, N(, 3)] arrays."""
    E, N = sc.E, sc.N
    out = dict(out_vel=np.zeros((E, N, 3)), n_neighbors=np.zeros((E, N), np.int32), n_buildings=np.zeros((E, N), np.int32),
               status=np.zeros((E, N), np.int32), slack=np.zeros((E, N)))
    for e in range(E):
        n_live = N if sc.drone_counts is None else int(sc.drone_counts[e])
        b = bld if bld.ndim == 2 else bld[e]
        if sc.cnt is not None:
            b = b[:int(sc.cnt[e])]   # (the records behind an env's count are fillers on the device)
        vel_of = None
        if mot is not None:
            ends, speed, leg = mot
            vel_of = lambda j, e=e, b=b: ref8.velocity(b[j], ends[e, j], speed[e, j], leg[e, j], DT)[:2]
        r = ref.orca_env(sc.pos[e], sc.vel[e], sc.rad[e], n_live, des[e], b, vel_of, **kw)
        for k, v in zip(("out_vel", "n_neighbors", "n_buildings", "status", "slack"), r):
            out[k][e] = v
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("E,N,nb_max,max_neighbors,max_buildings,drone_counts,what", CASES, ids=IDS)
def test_device_equals_the_restatement_bit_for_bit(E, N, nb_max, max_neighbors, max_buildings, drone_counts, what):
    sc = scene(E, N, nb_max, drone_counts)
    env, motion = city.live_env(sc)
    bld, mot = city.now(sc, motion)
    kw = dict(PAR, max_neighbors=max_neighbors, max_buildings=max_buildings)
    out, diag = env.orca_vel(diagnostics=True, **kw)
    want = restate(sc, env.des_vel().cpu().numpy(), bld, mot, **kw)
    live = np.ones((E, N), bool) if drone_counts is None else np.arange(N)[None, :] < np.array(drone_counts)[:, None]
    for k in ("n_neighbors", "n_buildings", "status"):
        assert np.array_equal(diag[k].cpu().numpy(), want[k]), k
    assert np.array_equal(bits(diag["slack"].cpu().numpy()), bits(want["slack"]))
    assert np.array_equal(bits(out.cpu().numpy()), bits(want["out_vel"]))
    st = want["status"]
    print(what, "status 1 / 2 / 3:", [(st == s).sum() for s in (1, 2, 3)], "status 3 at a lane >= 64:", (st[:, 64:] == 3).sum())
    assert (st[live] >= 1).all() and (st[~live] == 0).all()
    for k in diag:                                                   # rule 7: ghost rows are zeros
        assert not diag[k].cpu().numpy()[~live].any(), k
    assert not out.cpu().numpy()[~live].any()
    assert np.isfinite(out.cpu().numpy()).all()
    if what in STATUS_FLOORS:
        f1, f2, f3, f3hi = STATUS_FLOORS[what]
        assert (st == 1).sum() >= f1 and (st == 2).sum() >= f2 and (st == 3).sum() >= f3 and (st[:, 64:] == 3).sum() >= f3hi
        assert (want["slack"][st == 3] > 0.0).any()
    if N >= 64 and drone_counts is None:
        assert want["n_neighbors"].max() == max_neighbors and (want["n_neighbors"][live] == max_neighbors).mean() > 0.5
    if max_buildings == 0 or nb_max == 0:
        assert not want["n_buildings"].any()
    else:
        assert want["n_buildings"].max() >= 1 and want["n_buildings"].max() <= max_buildings
    if nb_max and nb_max > 1:
        assert (want["n_buildings"][E - 1] == 0).all()               # a set of fillers alone
    if nb_max == 129:
        assert want["n_buildings"].max() == 8
    if mot is not None and max_buildings and N >= 64 and nb_max >= 3:   # the motion shows: standing records give other bits
        still = restate(sc, env.des_vel().cpu().numpy(), bld, None, **kw)
        assert not np.array_equal(bits(still["out_vel"]), bits(want["out_vel"]))
    env.close()


def converter_state(E, N, seed):
    rng = np.random.default_rng(seed)
    speed, yaw, pitch = rng.uniform(0.0, 2.0, (E, N)), rng.uniform(0.0, 360.0, (E, N)), rng.uniform(-80.0, 80.0, (E, N))
    speed[:, ::7] = 0.0
    cy, sy = np.cos(np.radians(yaw)), np.sin(np.radians(yaw))
    cp, sp = np.cos(np.radians(pitch)), np.sin(np.radians(pitch))
    v = np.stack([speed * cp * cy, speed * cp * sy, speed * sp], axis=-1)
    w = rng.uniform(-1.5, 1.5, (E, N, 3))
    near = rng.uniform(size=(E, N)) < 0.5                            # half of them near the current velocity: unclipped
    w[near] = v[near] + rng.uniform(-0.3, 0.3, (int(near.sum()), 3))
    w[:, ::11] = 0.0
    return v, yaw, pitch, w


@pytest.mark.parametrize("E,N,drone_counts", [(3, 65, None), (4, 64, (64, 1, 30, 7))], ids=["full", "counted"])
def test_velocity_command_against_the_restatement(E, N, drone_counts):
    """rvo3d_vel_command: every action within orca_ref.CONVERTER_TOL of the restatement's (atan2 and asin are the device
    library's), the clipped bits exactly (rows whose unclipped value lies within the tolerance of +-1 are not judged:
    counted, at most 1 %), ghost rows zero."""
    sc = city.scene(E, N, 3, drone_counts)
    env, _ = city.live_env(sc)
    v, yaw, pitch, w = converter_state(E, N, 5 + N)
    env.set_state(vel=v, yaw=yaw, pitch=pitch)
    act, clipped = env.velocity_command(torch.as_tensor(w, device="cuda"), return_clipped=True)
    act, clipped = act.cpu().numpy(), clipped.cpu().numpy()
    assert torch.equal(env.velocity_command(w), torch.as_tensor(act, device="cuda"))
    live = np.ones((E, N), bool) if drone_counts is None else np.arange(N)[None, :] < np.array(drone_counts)[:, None]
    worst, edge, seen = 0.0, 0, np.zeros(3, int)
    for e in range(E):
        for i in range(N):
            if not live[e, i]:
                assert not act[e, i].any() and clipped[e, i] == 0
                continue
            a, b = ref.vel_command(v[e, i], yaw[e, i], pitch[e, i], w[e, i])
            worst = max(worst, float(np.abs(act[e, i] - a).max()))
            raw = ref.vel_command(v[e, i], yaw[e, i], pitch[e, i], w[e, i], clip=False)[0]
            if any(abs(abs(x) - 1.0) <= ref.CONVERTER_TOL for x in raw):
                edge += 1
                continue
            assert clipped[e, i] == b, (e, i, clipped[e, i], b, raw)
            seen += [b >> k & 1 for k in range(3)]
    print("largest |device - restatement| of an action:", worst, "tolerance", ref.CONVERTER_TOL, "clipped", seen, "edge", edge)
    assert worst <= ref.CONVERTER_TOL
    assert edge * 100 <= E * N and (seen >= 5).all()
    env.close()


def raw(env, out, motion="attached", dt=DT, diag=None, **kw):
    """The raw entry point.  motion: "attached" (the env's), None, or a _lib.BuildingMotionArgs."""
    par = dict(PAR, max_neighbors=10, max_buildings=4)
    par.update(kw)
    names = ("n_neighbors", "n_buildings", "status", "slack")
    a = _lib.OrcaArgs(par["time_horizon"], par["time_step"], par["max_speed"], par["pref_speed"], par["neighbor_dist"],
                      par["max_neighbors"], par["max_buildings"], par["reach"], par["below"], par["clear_xy"],
                      None if out is None else out.data_ptr(), *[None if diag is None else diag[n].data_ptr() for n in names])
    m = motion
    if isinstance(motion, str):
        m = None if env._motion is None else env._motion._args
    return _lib.lib().rvo3d_orca_vel(env._h, C.byref(a) if par.get("args", True) else None,
                                     None if m is None else C.byref(m), dt, env._stream())


def test_refused_calls_write_nothing():
    sc = city.scene(3, 5, 3)
    env, motion = city.live_env(sc)
    E, N = 3, 5
    out = torch.full((E, N, 3), -7.0, dtype=torch.float64, device="cuda")
    diag = {n: torch.full((E, N), -7, dtype=torch.int32, device="cuda") for n in ("n_neighbors", "n_buildings", "status")}
    diag["slack"] = torch.full((E, N), -7.0, dtype=torch.float64, device="cuda")
    inf, nan = float("inf"), float("nan")
    bad = [dict(time_horizon=0.0), dict(time_horizon=nan), dict(time_step=0.0), dict(time_step=inf), dict(max_speed=-1.0),
           dict(max_speed=nan), dict(pref_speed=-0.5), dict(pref_speed=inf), dict(neighbor_dist=0.0), dict(neighbor_dist=nan),
           dict(max_neighbors=0), dict(max_neighbors=17), dict(max_buildings=-1), dict(max_buildings=9), dict(reach=0.0),
           dict(reach=inf), dict(below=-1.0), dict(below=nan), dict(clear_xy=-1.0), dict(clear_xy=inf), dict(dt=-1.0),
           dict(dt=inf), dict(dt=nan), dict(args=False)]
    codes = set()
    for kw in bad:
        rc = raw(env, out, diag=diag, **kw)
        assert rc < 0, kw
        assert _lib.lib().rvo3d_last_error(), kw
        codes.add(rc)
    assert raw(env, None, diag=diag) in codes
    assert len(codes) == 1   # RVO3D_ERR_INVALID
    invalid = codes.pop()
    for field in ("ends", "speed", "leg"):
        m = _lib.BuildingMotionArgs(motion._args.ends, motion._args.speed, motion._args.leg)
        setattr(m, field, None)
        assert raw(env, out, motion=m, diag=diag) == invalid, field
    shared = city.scene(3, 64, None)
    env2, _ = city.live_env(shared)
    out_s = torch.full((3, 64, 3), -7.0, dtype=torch.float64, device="cuda")
    state = raw(env2, out_s, motion=motion._args)   # a motion on a handle without attached sets
    assert state < 0 and state != invalid
    with pytest.raises(_lib.RVO3DError):
        env.orca_vel(max_neighbors=17)
    # the converter's refusals
    L, w = _lib.lib(), torch.zeros((E, N, 3), dtype=torch.float64, device="cuda")
    assert L.rvo3d_vel_command(env._h, None, out.data_ptr(), None, env._stream()) == invalid
    assert L.rvo3d_vel_command(env._h, w.data_ptr(), None, None, env._stream()) == invalid
    assert L.rvo3d_vel_command(None, w.data_ptr(), out.data_ptr(), None, env._stream()) == invalid
    with pytest.raises(ValueError):
        env.velocity_command(torch.zeros((E, N, 2), device="cuda"))
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (out_s == -7.0).all()
    for k, v in diag.items():
        assert (v == -7).all(), k
    assert raw(env2, out_s, motion=None) == 0 and raw(env, out, diag=diag) == 0   # and the good calls go through
    torch.cuda.synchronize()
    assert not (out == -7.0).any() and not (out_s == -7.0).any() and (diag["status"] >= 1).all()
    env.close()
    env2.close()
