"""The building-aware classical RVO velocity on the device (include/rvo3d.h: rvo3d_rvo_vel_city) against the plain-Python
restatement (tests/rvo_city_ref.py), bit for bit and without exemptions: blocked_mask, n_gated and tier from the state,
out_vel from the restatement's selection made on the device's own live_mask, cone_mask, tc_min and env.des_vel(); against
rvo3d_rvo_vel where no building passes the gate (rule 5); planted drones; the argument table.

Shapes (CASES): N 5 / 64 / 65 / 130 - part of a wave, a full wave, the wave seam, three waves; E 3..6; nb_max 0 (the empty
shared list), 1, 3 and T + 1 = 129 at N = 65 (two tiles); per-env sets with unequal counts, one of them 0, and fillers; the
shared list; a counted handle with ghost rows; acceler 0, 0.5 and 1 (64 candidates); one vmax component 0; patrols with
static, arriving and cruising records, advanced MOVES times through rvo3d_move_env_buildings.

The second pass of rvo_city_body - the workgroup-wide vote, the lanes that wait at load_tile's barriers, the tb[4] minima
carried across tiles - has a scene of its own (moving_city_case.second_pass_scene: a counted handle, N 130, nb_max 193 =
T + 1 at T = 192, acceler 1).  The restatement on the CPU (tests/test_moving_city_host.py) gives there, and the test
asserts from the restatement of the device's own masks:

    tier-3 lanes   two distinct tb   ... at lane >= 64   least tb from record 192   first tile alone differs   mixed envs
    137            36                21 (>= 10)          2 (>= 1)                   2 (>= 1)                   1 (>= 1)

"least tb from record 192": the winning candidate's minimum over the buildings comes from the one record of the second
tile; "first tile alone differs": the lane's velocity is another one when tb is taken from records 0 .. 191 only - what a
second pass that read only the first tile would write, so such a kernel fails the bit-for-bit comparison (tried once: a
library built that way fails this test and passes every one of the CASES); "mixed envs": a wave without a tier-3 lane
beside one with (env 1's first wave flies over every roof).  Two of the CASES assert floors of their own tier-3 figures
(119 lanes, 16 of them with two distinct tb, at the wave seam; 12 lanes at three waves)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, BuildingMotion, World, _lib
import building_rows_moving_ref as ref8
import moving_city_case as mc
import rvo_city_ref as ref

pytestmark = pytest.mark.gpu
MAP = (20.0, 16.0, 8.0)
DT = 1.0
MOVES = 3
# (E, N, nb_max, acceler, vmax, drone counts, what): nb_max None - the shared list of 3, 0 - the empty shared list
CASES = [
    (3, 5, 3, 1.0, (2.0, 2.0, 2.0), None, "part of a wave, 64 candidates"),
    (4, 64, 1, 0.5, (2.0, 0.0, 2.0), None, "a full wave, one record, a vmax component 0: no candidates"),
    (3, 65, 129, 0.5, (2.0, 2.0, 2.0), None, "the wave seam, two tiles"),
    (3, 130, 3, 1.0, (2.0, 2.0, 1.0), None, "three waves"),
    (5, 64, 3, 1.0, (2.0, 2.0, 2.0), (64, 1, 30, 64, 7), "a counted handle"),
    (6, 65, 3, 0.0, (2.0, 2.0, 2.0), (65, 64, 1, 33, 65, 2), "counted across the seam, acceler 0: no candidates"),
    (3, 64, None, 0.5, (2.0, 2.0, 2.0), None, "the shared list"),
    (4, 5, 0, 1.0, (2.0, 2.0, 2.0), None, "no buildings at all"),
]
IDS = [c[-1] for c in CASES]
# floors of (tier-3 lanes, those whose blocked candidates have at least two distinct tb); the CPU counts 119 / 16 and 12 / 0
TIER3_FLOORS = {"the wave seam, two tiles": (60, 8), "three waves": (6, 0)}


def routes(E, N):
    wp = np.zeros((E, N, 2, 3))
    wp[:, :, 0] = [1.0, 1.0, 1.0]
    wp[:, :, 1] = [15.0, 9.0, 5.0]
    return wp, np.full((E, N), 2, np.int32)


@functools.lru_cache(maxsize=None)
def scene(E, N, nb_max, drone_counts=None):
    rng = np.random.default_rng(E * 1000 + N + 7 * (nb_max or 0))
    pos = rng.uniform(0.0, 1.0, (E, N, 3)) * np.array(MAP)
    ang, spd = rng.uniform(0, 2 * np.pi, (E, N)), rng.uniform(0.0, 2.0, (E, N))
    vel = np.stack([spd * np.cos(ang), spd * np.sin(ang), rng.uniform(-1, 1, (E, N))], axis=-1)
    vel[:, ::5] = 0.0
    rad = np.round(rng.uniform(0.1, 0.4, (E, N)), 3)
    wp, n_points = routes(E, N)
    dc = None if drone_counts is None else np.array(drone_counts, np.int32)
    sc = types.SimpleNamespace(E=E, N=N, pos=pos, vel=vel, rad=rad, drone_counts=dc, cnt=None, ends=None, speed=None)
    draw = lambda shape: np.concatenate([rng.uniform(0, MAP[0], shape + (1,)), rng.uniform(0, MAP[1], shape + (1,)),
                                         rng.uniform(0, MAP[2] + 2, shape + (1,)), rng.uniform(0.3, 1.5, shape + (1,))], axis=-1)
    if not nb_max:   # a shared list
        sc.bld0 = draw((3,)) if nb_max is None else np.zeros((0, 4))
        sc.world = World(wp, n_points, np.array(MAP), sc.bld0, None, dc)
        return sc
    sc.bld0 = draw((E, nb_max))
    sc.cnt = np.full(E, max(nb_max - 1, 1), dtype=np.int32)
    sc.cnt[0], sc.cnt[E - 1] = nb_max, 0
    sc.world = World(wp, n_points, np.array(MAP), sc.bld0, sc.cnt, dc)
    ends = np.zeros((E, nb_max, 2, 2))
    ends[:, :, 0] = sc.bld0[..., :2]
    ends[:, :, 1] = sc.bld0[..., :2] + rng.uniform(-6, 6, (E, nb_max, 2))
    speed = rng.uniform(0.3, 1.5, (E, nb_max))
    speed[:, ::3] = 0.0                                            # static records
    if nb_max > 1:                                                 # one that arrives with the next move after MOVES
        ends[:, 1, 1], speed[:, 1] = sc.bld0[:, 1, :2] + [2.1, 2.8], 1.0   # 3.5 m away at 1 m per step
    if nb_max > 2:                                                 # ... and one still under way: 10 m to go at 1 m per step
        ends[:, 2, 1], speed[:, 2] = sc.bld0[:, 2, :2] + [6.0, 8.0], 1.0
    sc.ends, sc.speed = ends, speed
    return sc


def live_env(sc):
    """The env of the scene, its patrols attached and advanced MOVES times, in the scene's state."""
    env = BatchedDroneEnv(sc.world, neighbors_num=3, radius=sc.rad)
    motion = None
    if sc.ends is not None:
        motion = BuildingMotion(sc.ends, sc.speed, dt=DT)
        env.attach_building_motion(motion)
        for _ in range(MOVES):
            motion.advance()
    env.set_state(pos=sc.pos, vel=sc.vel)
    return env, motion


def now(sc, motion):
    """(buildings, motion triple or None) as the device holds them now."""
    if motion is None:
        return sc.bld0, None
    return motion.buildings.cpu().numpy(), (sc.ends, sc.speed, motion.leg.cpu().numpy())


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def restate(sc, env, diag, bld, mot, **kw):
    des = env.des_vel().cpu().numpy()
    return ref.rvo_city_ref(sc.pos, sc.vel, sc.rad, bld, u64(diag["live_mask"]), u64(diag["cone_mask"]),
                            diag["tc_min"].cpu().numpy(), des, motion=mot, dt=DT, counts=sc.drone_counts,
                            building_counts=sc.cnt, **kw)


@pytest.mark.parametrize("E,N,nb_max,acceler,vmax,drone_counts,what", CASES, ids=IDS)
def test_device_equals_the_restatement_bit_for_bit(E, N, nb_max, acceler, vmax, drone_counts, what):
    sc = scene(E, N, nb_max, drone_counts)
    env, motion = live_env(sc)
    bld, mot = now(sc, motion)
    if mot is not None and nb_max > 1:   # the motion has a static, an arriving and a cruising record in every env with two
        br = {ref8.velocity(bld[0, j], sc.ends[0, j], sc.speed[0, j], mot[2][0, j], DT)[2] for j in range(int(sc.cnt[0]))}
        assert br == {0, 1, 2}, br
    kw = dict(vmax=vmax, acceler=acceler, horizon=5.0, reach=10.0, below=1.0, clear_xy=0.25, clear_z=0.5)
    out, diag = env.rvo_vel_city(diagnostics=True, **kw)
    want = restate(sc, env, diag, bld, mot, **kw)
    live = np.ones((E, N), bool) if drone_counts is None else np.arange(N)[None, :] < np.array(drone_counts)[:, None]
    assert np.array_equal(u64(diag["live_mask"]), want["live_mask"])        # (rule 0's candidates and live set)
    assert np.array_equal(u64(diag["blocked_mask"]), want["blocked_mask"])
    assert np.array_equal(diag["n_gated"].cpu().numpy(), want["n_gated"])
    assert np.array_equal(diag["tier"].cpu().numpy(), want["tier"])
    assert np.array_equal(bits(out.cpu().numpy()), bits(want["out_vel"]))
    tier = want["tier"]
    assert (tier[live] >= 1).all() and (tier[~live] == 0).all()
    if what in TIER3_FLOORS:   # the second pass is exercised: tier-3 lanes, and lanes whose candidates hit at different times
        lanes, two = TIER3_FLOORS[what]
        assert int((tier == 3).sum()) >= lanes, int((tier == 3).sum())
        assert two == 0 or mc.distinct_tb_lanes(sc, bld, mot, tier, u64(diag["live_mask"]), kw) >= two
    for k in diag:                                                           # rule 4: ghost rows are zeros
        assert not diag[k].cpu().numpy()[~live].any(), k
    assert not out.cpu().numpy()[~live].any()
    if acceler == 0.0 or 0.0 in vmax:   # np.arange(lo, lo, 0.5) is empty: no candidate, as in rvo3d_rvo_vel
        assert (tier[live] == 4).all() and not want["live_mask"].any()
    elif nb_max is None or nb_max:
        assert want["blocked_mask"].any() and want["n_gated"].max() >= 1 and (tier == 1).any()
    if nb_max and nb_max > 1:
        assert (want["n_gated"][E - 1] == 0).all()                           # a set of fillers alone
    else:
        assert nb_max != 0 or not want["n_gated"].any()
    # a second call with nothing in reach: the drone side does not depend on the buildings, and the row is rvo_vel's
    out0, diag0 = env.rvo_vel_city(diagnostics=True, **dict(kw, reach=1e-300))
    for k in ("live_mask", "cone_mask", "tc_min"):
        assert torch.equal(diag0[k].view(torch.int64), diag[k].view(torch.int64)), k
    assert not diag0["n_gated"].any() and not diag0["blocked_mask"].any()
    plain = env.rvo_vel(vmax=vmax, acceler=acceler)
    assert torch.equal(out0.view(torch.int64), plain.view(torch.int64))      # rule 5
    t0 = diag0["tier"].cpu().numpy()
    assert np.isin(t0[live], [1, 2, 4]).all()


def test_the_second_pass_across_waves_and_tiles():
    """moving_city_case.second_pass_scene, bit for bit against the restatement, and the figures of the module docstring
    from the restatement's output: tier-3 lanes beyond the first wave with distinct tb, a winner decided by the record of
    the second tile, and an env in which one wave needs no second pass while the others do."""
    sc = mc.second_pass_scene()
    assert (sc.N, sc.bld0.shape[1], mc.PASS_MOVES) == (130, 193, MOVES) and MAP == mc.PASS_MAP
    env, motion = live_env(sc)
    assert "counted" in env.kernel_name()
    bld, mot = now(sc, motion)
    b_ref, leg_ref = mc.second_pass_now()
    assert np.array_equal(bits(bld), bits(b_ref)) and np.array_equal(mot[2], leg_ref)
    kw = mc.PASS_KW
    out, diag = env.rvo_vel_city(diagnostics=True, **kw)
    want = restate(sc, env, diag, bld, mot, **kw)
    live = np.arange(sc.N)[None, :] < sc.drone_counts[:, None]
    assert np.array_equal(u64(diag["live_mask"]), want["live_mask"])
    assert np.array_equal(u64(diag["blocked_mask"]), want["blocked_mask"])
    assert np.array_equal(diag["n_gated"].cpu().numpy(), want["n_gated"])
    assert np.array_equal(diag["tier"].cpu().numpy(), want["tier"])
    assert np.array_equal(bits(out.cpu().numpy()), bits(want["out_vel"]))
    for k in diag:
        assert not diag[k].cpu().numpy()[~live].any(), k
    assert not out.cpu().numpy()[~live].any()
    assert (want["n_gated"][1, :64] == 0).all() and (want["n_gated"][0, :sc.drone_counts[0]] > 0).all()
    fig = mc.second_pass_figures(sc, bld, mot[2], want["tier"], u64(diag["live_mask"]), env.des_vel().cpu().numpy())
    print(fig)
    assert fig["distinct_64"] >= 10 and fig["from_192"] >= 1 and fig["mixed_envs"] >= 1, fig
    assert fig["first_tile_differs"] >= 1, fig


def raw(env, out, motion="attached", dt=DT, diag=None, **kw):
    """The raw entry point.  motion: "attached" (the env's), None, or a _lib.BuildingMotionArgs."""
    par = dict(vmax=(2.0, 2.0, 2.0), acceler=0.5, reach=10.0, below=1.0, horizon=5.0, clear_xy=0.0, clear_z=0.0)
    par.update(kw)
    names = ("live_mask", "cone_mask", "blocked_mask", "tc_min", "n_gated", "tier")
    a = _lib.RvoCityArgs((C.c_double * 3)(*par["vmax"]), par["acceler"], par["reach"], par["below"], par["horizon"],
                         par["clear_xy"], par["clear_z"], None if out is None else out.data_ptr(),
                         *[None if diag is None else diag[n].data_ptr() for n in names])
    m = motion
    if isinstance(motion, str):
        m = None if env._motion is None else env._motion._args
    return _lib.lib().rvo3d_rvo_vel_city(env._h, C.byref(a) if par.get("args", True) else None,
                                         None if m is None else C.byref(m), dt, env._stream())


def diag_buffers(E, N, fill=0):
    t = {n: torch.full((E, N), fill, dtype=torch.int64, device="cuda") for n in ("live_mask", "cone_mask", "blocked_mask")}
    t["tc_min"] = torch.full((E, N), float(fill), dtype=torch.float64, device="cuda")
    t["n_gated"] = torch.full((E, N), fill, dtype=torch.int32, device="cuda")
    t["tier"] = torch.full((E, N), fill, dtype=torch.int32, device="cuda")
    return t


def test_planted_drones():
    """Env 0 of three, five buildings (h 7 but D: 6), five drones; acceler 0.5, so candidate 7 is the current velocity.
    Drone 0 flies head-on at the standing A: 7 is blocked.  Drone 1 hovers in the path of B, which comes at it at 1 m per
    step: blocked only with the motion.  Drone 2 flies alongside C at C's velocity: free only with the motion.  Drone 3
    climbs at D: at 1 m per step it clears the roof (7 free), at 0.5 it does not (6 blocked).  Drone 4 is inside E's disk
    below its roof: every live candidate is blocked, tier 3."""
    E, N, nb = 3, 5, 5
    bld0 = np.zeros((E, nb, 4))
    bld0[:] = [[8.0, 8.0, 7.0, 1.0], [16.0, 3.0, 7.0, 1.0], [4.0, 12.0, 7.0, 1.0], [8.0, 14.5, 6.0, 1.0], [16.0, 8.0, 7.0, 2.0]]
    cnt = np.array([nb, 0, 2], np.int32)
    ends = np.zeros((E, nb, 2, 2))
    ends[:, :, 0] = ends[:, :, 1] = bld0[..., :2]
    speed = np.zeros((E, nb))
    ends[0, 1], speed[0, 1] = [[16.0, 3.0], [4.0, 3.0]], 1.0     # B: after three moves at (13, 3), velocity (-1, 0)
    ends[0, 2], speed[0, 2] = [[4.0, 12.0], [16.0, 12.0]], 0.5   # C: at (5.5, 12), velocity (0.5, 0)
    pos = np.zeros((E, N, 3))
    pos[:] = [[2.0, 8.0, 3.0], [9.0, 3.0, 3.0], [4.0, 12.0, 3.0], [2.0, 14.5, 3.0], [16.5, 8.0, 2.0]]
    vel = np.zeros((E, N, 3))
    vel[:] = [[1.5, 0.0, 0.0], [0.0, 0.0, 0.5], [0.5, 0.0, 0.25], [1.0, 0.0, 1.0], [0.5, 0.5, 0.5]]
    wp, n_points = routes(E, N)
    sc = types.SimpleNamespace(world=World(wp, n_points, np.array(MAP), bld0, cnt), rad=np.full((E, N), 0.2), ends=ends,
                               speed=speed, pos=pos, vel=vel, drone_counts=None, cnt=cnt, bld0=bld0)
    env, motion = live_env(sc)
    b = motion.buildings.cpu().numpy()
    assert b[0, 1, :2].tolist() == [13.0, 3.0] and b[0, 2, :2].tolist() == [5.5, 12.0]
    out, d = env.rvo_vel_city(diagnostics=True)
    blk, live, tier = u64(d["blocked_mask"])[0], u64(d["live_mask"])[0], d["tier"].cpu().numpy()[0]
    assert (live >> np.uint64(7) & np.uint64(1)).all()
    still = diag_buffers(E, N)
    out2 = torch.zeros_like(out)
    assert raw(env, out2, motion=None, diag=still) == 0           # the same records, every one standing
    blk0 = u64(still["blocked_mask"])[0]
    bit = lambda m, c: int(m) >> c & 1
    assert bit(blk[0], 7) and bit(blk0[0], 7)
    assert bit(blk[1], 7) and not bit(blk0[1], 7) and blk0[1] == 0
    assert not bit(blk[2], 7) and bit(blk0[2], 7)
    assert not bit(blk[3], 7) and bit(blk[3], 6)
    assert blk[4] == live[4] != 0 and tier[4] == 3 and out.cpu().numpy()[0, 4].any()
    assert (d["n_gated"].cpu().numpy()[1] == 0).all()
    want = restate(sc, env, d, b, (ends, speed, motion.leg.cpu().numpy()))
    assert np.array_equal(bits(out.cpu().numpy()), bits(want["out_vel"])) and np.array_equal(tier, want["tier"][0])
    want0 = restate(sc, env, still, b, None)
    assert np.array_equal(bits(out2.cpu().numpy()), bits(want0["out_vel"])) and np.array_equal(blk0, want0["blocked_mask"][0])


def test_argument_table_and_refused_calls_write_nothing():
    sc = scene(3, 5, 3)
    env, motion = live_env(sc)
    E, N = 3, 5
    out = torch.full((E, N, 3), -7.0, dtype=torch.float64, device="cuda")
    diag = diag_buffers(E, N, fill=-7)
    inf, nan = float("inf"), float("nan")
    bad = [dict(acceler=-0.1), dict(acceler=1.5), dict(acceler=nan), dict(reach=0.0), dict(reach=inf), dict(reach=nan),
           dict(below=-1.0), dict(below=nan), dict(horizon=0.0), dict(horizon=-1.0), dict(horizon=inf), dict(horizon=nan),
           dict(clear_xy=-1.0), dict(clear_xy=inf), dict(clear_z=-1.0), dict(clear_z=nan), dict(dt=-1.0), dict(dt=inf),
           dict(dt=nan), dict(args=False)]
    codes = set()
    for kw in bad:
        rc = raw(env, out, diag=diag, **kw)
        assert rc < 0, kw
        codes.add(rc)
    assert raw(env, None, diag=diag) in codes
    assert len(codes) == 1   # RVO3D_ERR_INVALID
    invalid = codes.pop()
    for field in ("ends", "speed", "leg"):
        m = _lib.BuildingMotionArgs(motion._args.ends, motion._args.speed, motion._args.leg)
        setattr(m, field, None)
        assert raw(env, out, motion=m, diag=diag) == invalid, field
    for dt in (-1.0, nan):
        assert raw(env, out, motion=None, dt=dt, diag=diag) == invalid
    shared = scene(3, 64, None)
    env2, _ = live_env(shared)
    out_s = torch.full((3, 64, 3), -7.0, dtype=torch.float64, device="cuda")
    state = raw(env2, out_s, motion=motion._args)   # a motion on a handle without attached sets
    assert state < 0 and state != invalid
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (out_s == -7.0).all()
    for k, v in diag.items():
        assert (v == -7).all(), k
    assert raw(env2, out_s, motion=None) == 0 and raw(env, out, diag=diag) == 0   # and the good calls go through
    torch.cuda.synchronize()
    assert not (out == -7.0).any() and not (out_s == -7.0).any() and (diag["tier"] >= 1).all()
