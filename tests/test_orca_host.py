"""The host-testable halves of the ORCA velocity and the velocity command (include/rvo3d.h: rvo3d_orca_vel,
rvo3d_vel_command), no GPU needed:

  (a) tests/host/orca_check.hip - a stand-alone CPU program over the __host__ __device__ rules the kernel compiles
      (csrc/rvo3d_orca_rules.hpp) - against the plain-Python restatement tests/orca_ref.py, bit for bit: planes, velocities,
      counts, status and slack on seeded scenes with every branch planted; the argument-check table is its self-test;
  (b) properties of the restatement's results that do not depend on how the programs are coded: the speed ball, the
      planes, optimality against a sampled ball, reciprocity;
  (c) the converter against the oracle's kinematic step;
  (d) the closed loop: restatement -> converter -> the oracle's step on the circle swap tests/golden/rvo_orca_swap_scene.npz.

The program is built with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and run as a child process.

Status counts of SCENES (restatement, CPU; asserted as floors of 10 each below), lanes with status 1 / 2 / 3:
  default 13 / 101 / 18, few_kept 31 / 35 / 66, standing 33 / 0 / 99 (max_speed 0), moving_wide 22 / 84 / 26; in all 99 / 220 / 209."""
import collections
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import oracle as orc
import orca_ref as ref

CSRC = os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "orca_check.hip")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-O1",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
SCENE = os.path.join(ROOT, "tests", "golden", "rvo_orca_swap_scene.npz")
TOL = 1e-9   # derived, not measured: fp64 steps on O(10) operands, amplified by at most
             # 1 / |n_j x n_i| with |.|^2 > EPS = 1e-5 - several orders above 1e-16 * 10 * 300


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("orca") / "orca_check")
    subprocess.check_call([hipcc] + FLAGS + ["-I", CSRC, "-o", out, SRC])
    return out


PAR = dict(time_horizon=5.0, time_step=1.0, max_speed=2.0, pref_speed=1.0, neighbor_dist=10.0, max_neighbors=10,
           max_buildings=4, reach=10.0, below=1.0, clear_xy=0.0)


def _run(exe, tmp_path, drones, bld, motion=None, dt=1.0, par=PAR):
    n, nb = len(drones), len(bld)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, nb, motion is not None, par["max_neighbors"], par["max_buildings"]], dtype=np.int32).tobytes())
        f.write(np.array([par[k] for k in ("time_horizon", "time_step", "max_speed", "pref_speed", "neighbor_dist", "reach",
                                           "below", "clear_xy")] + [dt], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(drones, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(bld, dtype=np.float64).tobytes())
        if motion is not None:
            ends, speed, leg = motion
            f.write(np.ascontiguousarray(ends, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(speed, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(leg, dtype=np.uint8).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    raw = open(fout, "rb").read()
    ints = np.frombuffer(raw, np.int32, n * 3, 0).reshape(n, 3)
    vals = np.frombuffer(raw, np.float64, n * 4, 12 * n).reshape(n, 4)
    planes = np.frombuffer(raw, np.float64, n * 24 * 6, 12 * n + 32 * n).reshape(n, 24, 6)
    return ints, vals, planes


def host_scene(seed=11):
    """132 drones (pos, vel, r, des) and 14 buildings with patrols on a 30 x 30 x 10 map.  Planted: drones 0 and 1 at the same
    place with the same velocity (a zero-length w, the normal (1, 0, 0)); 2 and 3 head-on, 4 and 5 crossing at right
    angles, 6 and 7 overlapping; drones 100..131 in a ball of 0.8 m round (8, 8, 5) with radii of 0.5: they overlap, have
    more than 16 neighbours each and no common point of their planes (the fallback).  Building 0 stands 3 m from drone 8,
    roof above it (passes); building 1 is 10.5 m from drone 8 (fails the distance half), building 2 is 2 m from drone 8 with
    its roof 1 m below it (fails the height half; below = 1), building 3 is a filler, building 4 patrols towards drone 9."""
    rng = np.random.default_rng(seed)
    n, nb = 132, 14
    pos = rng.uniform(0, 1, (n, 3)) * [30.0, 30.0, 10.0]
    ang, spd = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.0, 1.5, n)
    vel = np.stack([spd * np.cos(ang), spd * np.sin(ang), rng.uniform(-0.5, 0.5, n)], axis=-1)
    rad = np.round(rng.uniform(0.15, 0.4, n), 3)
    d = rng.normal(size=(n, 3))
    des = np.round(d / np.linalg.norm(d, axis=1, keepdims=True), 3)
    des[::9] = 0.0
    c = rng.normal(size=(32, 3))
    pos[100:] = [8.0, 8.0, 5.0] + 0.8 * c / np.linalg.norm(c, axis=1, keepdims=True) * rng.uniform(0, 1, (32, 1)) ** (1 / 3)
    rad[100:] = 0.5
    vel[100:] *= 0.3
    pos[0], pos[1], vel[0], vel[1] = [25.0, 25.0, 8.0], [25.0, 25.0, 8.0], [0.5, 0.25, 0.0], [0.5, 0.25, 0.0]
    pos[2], pos[3], vel[2], vel[3] = [20.0, 3.0, 3.0], [24.0, 3.0, 3.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]
    pos[4], pos[5], vel[4], vel[5] = [3.0, 20.0, 3.0], [6.0, 23.0, 3.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]
    pos[6], pos[7], vel[6], vel[7] = [3.0, 27.0, 8.0], [3.3, 27.0, 8.1], [0.2, 0.0, 0.0], [-0.1, 0.1, 0.0]
    des[2], des[3], des[4], des[5] = [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]
    bld = np.concatenate([rng.uniform(0, 30, (nb, 2)), rng.uniform(2, 12, (nb, 1)), rng.uniform(0.4, 2.0, (nb, 1))], axis=1)
    pos[8], pos[9] = [15.0, 15.0, 4.0], [22.0, 12.0, 3.0]
    bld[0], bld[1], bld[2] = [18.0, 15.0, 9.0, 1.0], [15.0, 25.5, 9.0, 1.0], [15.0, 13.0, 3.0, 0.5]
    bld[3] = [5.0, 5.0, -np.inf, 1.0]
    bld[4] = [26.0, 12.0, 9.0, 1.0]
    ends = np.zeros((nb, 2, 2))
    ends[:, 0] = bld[:, :2]
    ends[:, 1] = bld[:, :2] + rng.uniform(-6, 6, (nb, 2))
    speed = rng.uniform(0.3, 1.2, nb)
    speed[::3] = 0.0
    ends[4, 1], speed[4] = [16.0, 12.0], 1.0
    ends[3], speed[3] = np.nan, np.nan
    leg = np.ones(nb, np.uint8)
    drones = np.concatenate([pos, vel, rad[:, None], des], axis=1)
    return drones, bld, (ends, speed, leg)


SCENES = {
    "default": (PAR, False),
    "few_kept": (dict(PAR, max_neighbors=3, max_buildings=1, neighbor_dist=6.0, max_speed=0.3, pref_speed=0.3), True),
    "standing": (dict(PAR, max_speed=0.0), False),
    "moving_wide": (dict(PAR, clear_xy=0.5, time_horizon=3.0, max_neighbors=16, max_buildings=8, max_speed=1.5), True),
}
KW = ("time_horizon", "time_step", "neighbor_dist", "max_neighbors", "max_buildings", "reach", "below", "clear_xy")


def restate(par, moving, tally=None):
    """The restatement on host_scene: a list of orca_ref.orca_drone results."""
    import building_rows_moving_ref as ref8
    drones, bld, (ends, speed, leg) = host_scene()
    vel_of = (lambda j: ref8.velocity(bld[j], ends[j], speed[j], leg[j], 1.0)[:2]) if moving else (lambda j: (0.0, 0.0))
    pos, vel, rad, des = drones[:, :3], drones[:, 3:6], drones[:, 6], drones[:, 7:]
    kw = {k: par[k] for k in KW}
    return [ref.orca_drone(i, pos, vel, rad, len(drones), des[i], bld, vel_of, max_speed=par["max_speed"],
                           pref_speed=par["pref_speed"], tally=tally, **kw) for i in range(len(drones))]


_cache = {}


def restated(name):
    if name not in _cache:
        tally = collections.Counter()
        _cache[name] = (restate(*SCENES[name], tally=tally), tally)
    return _cache[name]


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


# ---- (a) ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SCENES))
def test_host_rules_equal_the_restatement(exe, tmp_path, name):
    """(a) planes, out_vel, n_neighbors, n_buildings, status and slack of the header's functions: the restatement's bits."""
    par, moving = SCENES[name]
    drones, bld, motion = host_scene()
    ints, vals, planes = _run(exe, tmp_path, drones, bld, motion if moving else None, 1.0, par)
    want, tally = restated(name)
    for i, w in enumerate(want):
        assert tuple(ints[i]) == (w["n_neighbors"], w["n_buildings"], w["status"]), (i, ints[i], w["status"])
        wp = np.zeros((24, 6))
        for k, (pt, nrm) in enumerate(w["planes"]):
            wp[k] = list(pt) + list(nrm)
        assert np.array_equal(bits(planes[i]), bits(wp)), (i, planes[i][:len(w["planes"])], wp[:len(w["planes"])])
        assert np.array_equal(bits(vals[i]), bits([w["slack"]] + list(w["v"]))), (i, vals[i], w["slack"], w["v"])
    assert np.isfinite(vals).all() and np.isfinite(planes).all()
    print(name, "status", collections.Counter(int(s) for s in ints[:, 2]), dict(tally))


def test_status_floors_and_planted_cases():
    """Every status on at least 10 lanes of every scene that can have it, every branch of rule 4 for drones and buildings,
    and the planted cases are what host_scene's comment says."""
    total = collections.Counter()
    for name in SCENES:
        want, tally = restated(name)
        st = collections.Counter(w["status"] for w in want)
        print(name, dict(st), dict(tally))
        total.update(st)
        assert st[1] >= 10 and st[3] >= 10, (name, st)
        if SCENES[name][0]["max_speed"] > 0.0:
            assert st[2] >= 10, (name, st)
        for b in range(3):
            assert tally["drone_branch%d" % b] >= 10, (name, tally)
        assert tally["building_branch0"] >= 3 and tally["building_branch1"] >= 3, (name, tally)
    print("in all", dict(total))
    want, _ = restated("default")
    drones, bld, _m = host_scene()
    assert want[0]["planes"][0][1] == (1.0, 0.0, 0.0) and want[1]["planes"][0][1] == (1.0, 0.0, 0.0)   # the zero-length w
    assert max(w["n_neighbors"] for w in want[100:]) == 10 and sum(w["status"] == 3 and w["slack"] > 0.0 for w in want[100:]) >= 10
    p8, r8 = drones[8, :3], drones[8, 6]
    assert ref.gate(p8, r8, bld[0], 10.0, 1.0)[0]
    assert not ref.gate(p8, r8, bld[1], 10.0, 1.0)[0] and bld[1, 2] > p8[2] - 1.0            # the distance half alone
    assert not ref.gate(p8, r8, bld[2], 10.0, 1.0)[0] and np.hypot(*(p8[:2] - bld[2, :2])) <= 10.0   # the height half alone
    assert not ref.gate(p8, r8, bld[3], 10.0, 1.0)[0]                                         # a filler
    moving, _ = restated("moving_wide")
    still = restate(dict(SCENES["moving_wide"][0]), False)
    assert moving[9]["planes"][0] != still[9]["planes"][0]                                    # the moving building shows
    assert max(w["n_neighbors"] for w in restated("moving_wide")[0]) == 16
    assert all(w["n_neighbors"] <= 3 and w["n_buildings"] <= 1 for w in restated("few_kept")[0])
    assert all(w["v"] == (0.0, 0.0, 0.0) or max(abs(x) for x in w["v"]) == 0.0 for w in restated("standing")[0])


def test_status_counts_of_the_device_scene():
    """The status floors tests/test_gpu_orca.py asserts on its "three waves" scene, from the CPU: the scene restated with
    des_vel as the unit vector towards the waypoint (the device rounds it to three decimals) and the patrols as they stand
    before their first move.  Counted: status 1 / 2 / 3 = 12 / 318 / 60, status 3 at a lane >= 64: 59; the floors are
    half of each."""
    import test_gpu_orca as g
    E, N, nb_max = 3, 130, 3
    sc = g.scene(E, N, nb_max)
    d = np.array([15.0, 9.0, 5.0]) - sc.pos
    des = d / np.linalg.norm(d, axis=-1, keepdims=True)
    bld = sc.bld0
    mot = (sc.ends, sc.speed, np.ones((E, nb_max), np.uint8))
    st = g.restate(sc, des, bld, mot, **dict(g.PAR, max_neighbors=16, max_buildings=4))["status"]
    counts = [int((st == s).sum()) for s in (1, 2, 3)] + [int((st[:, 64:] == 3).sum())]
    print("three waves on the CPU: status 1 / 2 / 3 and 3 at a lane >= 64:", counts)
    assert all(c >= 2 * f for c, f in zip(counts, g.STATUS_FLOORS["three waves"])), counts


def test_argument_table_and_hand_computed_cases(exe):
    """The program's self-test: every refusal of rvo3d_orca_vel's argument check, rule 4 branch by branch, the slots, the
    programs on cases with known answers and the converter."""
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    print(res.stderr)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "orca ok" in res.stdout


# ---- (b) ----------------------------------------------------------------------------------------------------------------------

def _arr(planes):
    if not planes:
        return np.zeros((0, 3)), np.zeros((0, 3))
    return np.array([p for p, _ in planes]), np.array([n for _, n in planes])


@pytest.mark.parametrize("name", list(SCENES))
def test_properties_of_the_result(name):
    """(b) |v| <= max_speed + 1e-9; every building plane holds to 1e-9 - on every lane whose building planes have a common
    point inside the speed ball at all (rule 6: where they have none, the program fails at a building plane and relaxes
    it: a speed ball too small to get away from a moving building, a drone inside two clearance disks; such lanes are
    counted, and the scene with standing buildings and the default parameters has none); for status 1 and 2 every drone plane
    holds; for status 1 the result is pref clipped to the ball; status 3 has a drone plane that does not hold."""
    par, _ = SCENES[name]
    want, _ = restated(name)
    ms = par["max_speed"]
    no_common_point = 0
    for i, w in enumerate(want):
        v, hard = np.array(w["v"]), w["n_buildings"]
        pts, nrm = _arr(w["planes"])
        assert math.sqrt(ref.dot(w["v"], w["v"])) <= ms + TOL, (i, w["v"])
        hold = ((v - pts) * nrm).sum(axis=1)
        if ref.lp3(w["planes"][:hard], hard, ms, w["pref"], False)[0] == hard:
            assert (hold[:hard] >= -TOL).all(), (i, hold[:hard])
        else:
            no_common_point += 1
        if w["status"] in (1, 2):
            assert (hold >= -TOL).all(), (i, w["status"], hold.min())
            assert w["slack"] == 0.0
        else:
            assert w["slack"] >= 0.0 and (hard == len(hold) or abs(max(0.0, -hold[hard:].min()) - w["slack"]) <= TOL)
        if w["status"] == 1:
            pref = np.array(w["pref"])
            ln = math.sqrt(ref.dot(w["pref"], w["pref"]))
            clipped = pref if ln <= ms else pref / ln * ms
            assert np.abs(v - clipped).max() <= TOL, (i, v, clipped)
    print(name, "lanes whose building planes have no common point in the ball:", no_common_point)
    if name == "default":
        assert no_common_point == 0


@pytest.mark.parametrize("name", [n for n in SCENES if SCENES[n][0]["max_speed"] > 0.0])
def test_optimality_against_a_sampled_ball(name):
    """(b) the speed ball on a grid of step max_speed / 20.  Status 2: no sample that satisfies all planes is nearer to pref
    than the result by more than 1e-9.  Status 3: no sample that satisfies the building planes has a smaller largest
    penetration over the drone planes than slack - 1e-9."""
    par, _ = SCENES[name]
    want, _ = restated(name)
    ms = par["max_speed"]
    g = np.arange(-20, 21) * (ms / 20.0)
    X = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    X = X[(X * X).sum(axis=1) <= ms * ms]
    seen = collections.Counter()
    for i, w in enumerate(want):
        if w["status"] == 1:
            continue
        pts, nrm = _arr(w["planes"])
        hard = w["n_buildings"]
        pen = (pts * nrm).sum(axis=1)[None, :] - X @ nrm.T          # n . (point - x), [samples, planes]
        if w["status"] == 2:
            ok = (pen <= 0.0).all(axis=1)
            if ok.any():
                best = np.sqrt(((X[ok] - np.array(w["pref"])) ** 2).sum(axis=1)).min()
                mine = math.sqrt(sum((a - b) ** 2 for a, b in zip(w["v"], w["pref"])))
                assert mine <= best + TOL, (i, mine, best)
                seen["status2"] += 1
        else:
            if ref.lp3(w["planes"][:hard], hard, ms, w["pref"], False)[0] != hard or hard == len(w["planes"]):
                continue
            ok = (pen[:, :hard] <= 0.0).all(axis=1)
            if ok.any():
                best = np.maximum(pen[ok][:, hard:].max(axis=1), 0.0).min()
                assert best >= w["slack"] - TOL, (i, best, w["slack"])
                seen["status3"] += 1
    print(name, dict(seen))
    assert seen["status2"] >= 10 and seen["status3"] >= 10


def _closest(p_i, p_j, v_i, v_j, tau):
    rel, dv = np.array(p_j) - np.array(p_i), np.array(v_j) - np.array(v_i)
    a = float(dv @ dv)
    t = 0.0 if a == 0.0 else min(max(-float(rel @ dv) / a, 0.0), tau)
    return float(np.linalg.norm(rel + t * dv))


@pytest.mark.parametrize("case", ["head_on", "crossing", "head_on_offset", "crossing_3d"])
def test_reciprocity(case):
    """(b) two drones, both applying their result: the closest approach over time_horizon is >= R - 1e-9."""
    pos = {"head_on": [[0.0, 0.0, 5.0], [6.0, 0.0, 5.0]], "crossing": [[0.0, 0.0, 5.0], [3.0, 3.0, 5.0]],
           "head_on_offset": [[0.0, 0.0, 5.0], [6.0, 0.3, 5.1]], "crossing_3d": [[0.0, 0.0, 5.0], [3.0, 3.0, 5.5]]}[case]
    vel = {"head_on": [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], "crossing": [[1.0, 0.0, 0.0], [0.0, -1.0, 0.0]],
           "head_on_offset": [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], "crossing_3d": [[1.0, 0.0, 0.1], [0.0, -1.0, -0.1]]}[case]
    rad = [0.4, 0.3]
    assert _closest(pos[0], pos[1], vel[0], vel[1], 5.0) < 0.7   # on a collision course as they fly now
    out, _, _, status, _ = ref.orca_env(np.array(pos), np.array(vel), rad, 2, np.array(vel), np.zeros((0, 4)), **{k: PAR[k] for k in KW})
    d = _closest(pos[0], pos[1], out[0], out[1], 5.0)
    print(case, "status", status, "closest approach", d)
    assert (status == 2).all()
    assert d >= 0.7 - TOL


# ---- (c) ----------------------------------------------------------------------------------------------------------------------

def converter_case(seed=3, n=64, clip=False):
    """(v, yaw, pitch, w) of n drones: without clip every command stays inside (-1, 1); with it the differences are large."""
    rng = np.random.default_rng(seed)
    speed, yaw, pitch = rng.uniform(0.0, 2.0, n), rng.uniform(0.0, 360.0, n), rng.uniform(-80.0, 80.0, n)
    speed[::8] = 0.0
    cy, sy, cp, sp = np.cos(np.radians(yaw)), np.sin(np.radians(yaw)), np.cos(np.radians(pitch)), np.sin(np.radians(pitch))
    v = np.stack([speed * cp * cy, speed * cp * sy, speed * sp], axis=-1)
    k = 2.5 if clip else 0.95
    nspeed = np.maximum(speed + rng.uniform(-k, k, n), 0.05)
    nyaw, npitch = yaw + rng.uniform(-90 * k, 90 * k, n), np.clip(pitch + rng.uniform(-90 * k, 90 * k, n), -89.0, 89.0)
    if not clip:
        npitch = np.clip(npitch, pitch - 85.0, pitch + 85.0)
    w = np.stack([nspeed * np.cos(np.radians(npitch)) * np.cos(np.radians(nyaw)),
                  nspeed * np.cos(np.radians(npitch)) * np.sin(np.radians(nyaw)), nspeed * np.sin(np.radians(npitch))], axis=-1)
    if clip:
        w[::16] = 0.0
    return v, yaw, pitch, w


CONVERTER_ERR, CONVERTER_TOL = ref.CONVERTER_ERR, ref.CONVERTER_TOL


def oracle_step_velocity(v, yaw, pitch, actions):
    """The oracle's kinematic step on n drones spread over a large map, far from their waypoints: the velocity behind it."""
    n = len(v)
    wp = np.zeros((1, n, 2, 3))
    wp[0, :, 0] = [[10.0 + 20.0 * (i % 8), 10.0 + 20.0 * (i // 8), 50.0] for i in range(n)]
    wp[0, :, 1] = wp[0, :, 0] + [0.0, 0.0, 40.0]
    env = orc.OracleEnv(wp, np.full((1, n), 2), [200.0, 200.0, 100.0], None, nm=2)
    env.reset()
    pos = wp[:, :, 0] + [3.0, 3.0, 0.0]
    env.set_state(pos=pos, vel=v[None], yaw=yaw[None], pitch=pitch[None])
    env.step(np.asarray(actions)[None])
    return env.get_state()["vel"][0]


def test_converter_against_the_step():
    """(c) for seeded (v, yaw, pitch, w) without clipping the oracle's kinematic step of the restated action gives w.
    Measured on this CPU comparison: the largest error 7.58e-15 (CONVERTER_ERR); the tolerance is ten times that, 7.58e-14
    (CONVERTER_TOL), which tests/test_gpu_orca.py uses for the device's converter as well."""
    v, yaw, pitch, w = converter_case()
    acts = []
    for i in range(len(v)):
        a, b = ref.vel_command(v[i], yaw[i], pitch[i], w[i])
        assert b == 0, (i, a)
        acts.append(a)
    got = oracle_step_velocity(v, yaw, pitch, acts)
    err = float(np.abs(got - w).max())
    print("converter: largest |step(command(w)) - w| =", err, "tolerance", CONVERTER_TOL)
    assert err <= 1e-9, "the formulas are wrong"
    assert err <= CONVERTER_TOL


def test_converter_clipped_bits():
    """(c) with clipping: the bits are exactly the components whose unclipped value lies outside [-1, 1] (computed here in
    numpy; components within 1e-9 of the edge are not judged), the clipped components are +-1 and a zero velocity keeps
    both angles."""
    v, yaw, pitch, w = converter_case(clip=True)
    seen = collections.Counter()
    for i in range(len(v)):
        a, b = ref.vel_command(v[i], yaw[i], pitch[i], w[i])
        wn = np.linalg.norm(w[i])
        raw = [wn - np.linalg.norm(v[i]), 0.0, 0.0]
        if wn > 0:
            raw[1] = ((np.degrees(np.arctan2(w[i, 1], w[i, 0])) - yaw[i] + 180.0) % 360.0 - 180.0) / 90.0
            raw[2] = (np.degrees(np.arcsin(np.clip(w[i, 2] / wn, -1, 1))) - pitch[i]) / 90.0
        else:
            assert a[1] == 0.0 and a[2] == 0.0
            seen["zero"] += 1
        for k in range(3):
            if abs(abs(raw[k]) - 1.0) <= 1e-9:
                continue
            assert bool(b >> k & 1) == (abs(raw[k]) > 1.0), (i, k, raw, a, b)
            assert abs(a[k] - np.clip(raw[k], -1.0, 1.0)) <= 1e-12, (i, k, raw, a)
            seen["clipped%d" % k] += b >> k & 1
    print(dict(seen))
    assert seen["zero"] >= 2 and all(seen["clipped%d" % k] >= 5 for k in range(3))


# ---- (d) ----------------------------------------------------------------------------------------------------------------------

def fly(scene, controller, steps, e=0):
    """Env e of the swap scene through the oracle's step: until a drone is done, all have finished or `steps` are flown.
    controller "des": des_vel through the converter; "orca": the restatement through the converter.  Returns (the least
    separation over the steps, steps flown, commands clipped, all finished)."""
    from rvo3d_amd.safety import safety_numpy
    wp, npts, ms, rad = scene["waypoints"][e:e + 1], scene["n_points"][e:e + 1], scene["map_size"], float(scene["radius"])
    kw = {k: (int(scene[k]) if k.startswith("max_n") or k == "max_buildings" else float(scene[k])) for k in KW}
    N = npts.shape[1]
    env = orc.OracleEnv(wp, npts, ms, None, nm=int(scene["nm"]), radius=np.full((1, N), rad))
    env.reset()
    env.set_state(yaw=scene["yaw"][e:e + 1])
    worst, clipped = np.inf, 0
    for t in range(steps):
        s, des = env.get_state(), env.des_vel()
        if controller == "des":
            w = des[0]
        else:
            w = ref.orca_env(s["pos"][0], s["vel"][0], np.full(N, rad), N, des[0], np.zeros((0, 4)),
                             max_speed=float(scene["max_speed"]), pref_speed=float(scene["pref_speed"]), **kw)[0]
        a = np.zeros((1, N, 3))
        for i in range(N):
            a[0, i], b = ref.vel_command(s["vel"][0, i], s["yaw"][0, i], s["pitch"][0, i], w[i])
            clipped += b != 0
        _, _, _, done, _, fin = env.step(a)
        sep = safety_numpy(env.get_state()["pos"], rad, ms, 0.5)[0]
        worst = min(worst, float(sep.min()))
        if done.any() or fin.all():
            return worst, t + 1, clipped, bool(fin.all())
    return worst, steps, clipped, False


def test_closed_loop_circle_swap():
    """(d) K drones on a circle, each routed to its antipode (two waypoints, radius 0.2, max_speed 1), started with the yaw
    of their route: ORCA through the converter never touches (sep > 0 at every step), clips no command and brings every
    drone to its goal; des_vel flown the same way touches in the middle."""
    scene = np.load(SCENE)
    steps = int(scene["steps"])
    assert float(scene["radius"]) == 0.2 and float(scene["max_speed"]) == 1.0 and scene["waypoints"].shape[2] == 2
    for e in range(scene["waypoints"].shape[0]):
        d_worst, d_steps, d_clipped, _ = fly(scene, "des", steps, e)
        o_worst, o_steps, o_clipped, o_fin = fly(scene, "orca", steps, e)
        print("env", e, "des_vel: sep", d_worst, "after", d_steps, "steps; orca: sep", o_worst, "over", o_steps, "steps, clipped",
              o_clipped, "finished", o_fin)
        assert d_worst <= 0.0
        assert o_worst > 0.0 and o_clipped == 0 and o_fin
