"""The host-testable halves of the building-aware classical RVO velocity (include/rvo3d.h: rvo3d_rvo_vel_city), no GPU
needed:

  (a) the gate of tests/rvo_city_ref.py - the plain-Python restatement the GPU tests compare the kernel against - against
      the reference's own reciprocal_vel_obs.preprocess (oracle.rvo_preprocess), decision for decision;
  (b) tests/host/rvo_city_check.hip - a stand-alone CPU program over the header's __host__ __device__ functions
      (csrc/rvo3d_rvo_city_kernels.hpp) - against the restatement, bit for bit, on seeded scenes with every branch of the
      swept test and all four tiers planted; the argument-check table is the program's self-test;
  (c) the closed loop: the whole controller restated in Python flies the fixture scene tests/golden/rvo_city_scene.npz
      through the oracle's step, next to des_vel.

The program is built with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and run as a child process."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import oracle as orc
import rvo_city_ref as ref

CSRC = os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "rvo_city_check.hip")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-O1",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
SCENE = os.path.join(ROOT, "tests", "golden", "rvo_city_scene.npz")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("rvo_city") / "rvo_city_check")
    subprocess.check_call([hipcc] + FLAGS + ["-I", CSRC, "-o", out, SRC])
    return out


# ---- (a) ----------------------------------------------------------------------------------------------------------------------

def test_gate_equals_the_reference_preprocess():
    """reach = 10, below = 1: the restatement keeps the buildings reciprocal_vel_obs.preprocess keeps.  Pairs within
    1e-12 (relative) of the distance gate or 1e-12 of the height gate may be exempt; they are counted and printed, and at
    most 1 % of the pairs may be.  Some pairs are planted right at the gates."""
    rng = np.random.default_rng(20250)
    nd, nb = 60, 80
    agents = rng.uniform(0, 1, (nd, 3)) * [40.0, 40.0, 12.0]
    bld = np.concatenate([rng.uniform(0, 40, (nb, 2)), rng.uniform(0, 14, (nb, 1)), rng.uniform(0.3, 2.5, (nb, 1))], axis=1)
    bld[0, :2], bld[1, :2] = agents[0, :2] + [6.0, 8.0], agents[1, :2] + [6.0, 8.000001]   # d == 10 exactly, d just above
    bld[2, 2], bld[3, 2] = agents[2, 2] - 1.0, agents[3, 2] - 0.999                        # h == p_z - 1: fails, just above
    bld[2, :2], bld[3, :2] = agents[2, :2] + 1.0, agents[3, :2] + 1.0
    exempt, kept, dropped_far, dropped_low = 0, 0, 0, 0
    for i in range(nd):
        want = orc.rvo_preprocess(agents[i], np.zeros((0, 3)), bld)[1]
        for j in range(nb):
            ok, ex, ey = ref.gate(agents[i], bld[j])
            d = np.hypot(ex, ey)
            if abs(d - 10.0) <= 1e-12 * 10.0 or abs(bld[j, 2] - (agents[i, 2] - 1.0)) <= 1e-12:
                exempt += 1
                continue
            assert ok == bool(want[j]), (i, j, d, bld[j], agents[i])
            kept += ok
            dropped_far += (not ok) and d > 10.0
            dropped_low += (not ok) and not bld[j, 2] > agents[i, 2] - 1.0
    print("pairs", nd * nb, "exempt", exempt, "kept", kept, "too far", dropped_far, "too low", dropped_low)
    assert exempt * 100 <= nd * nb
    assert kept > 200 and dropped_far > 200 and dropped_low > 200
    assert ref.gate(agents[3], bld[3])[0] and not ref.gate(agents[1], bld[1])[0]
    assert not ref.gate([0.0, 0.0, 3.0], [1.0, 1.0, -np.inf, 1.0])[0]   # a filler


# ---- (b) ----------------------------------------------------------------------------------------------------------------------

PAR = dict(reach=10.0, below=1.0, horizon=5.0, clear_xy=0.0, clear_z=0.0)


def _run(exe, tmp_path, drones, cnts, masks, bld, motion=None, dt=1.0, par=PAR):
    n, nb = len(drones), len(bld)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, nb, motion is not None], dtype=np.int32).tobytes())
        f.write(np.array([par["reach"], par["below"], par["horizon"], par["clear_xy"], par["clear_z"], dt],
                         dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(drones, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(cnts, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(masks, dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(bld, dtype=np.float64).tobytes())
        if motion is not None:
            ends, speed, leg = motion
            f.write(np.ascontiguousarray(ends, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(speed, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(leg, dtype=np.uint8).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    raw = open(fout, "rb").read()
    o = 0
    blocked = np.frombuffer(raw, np.uint64, n, o); o += 8 * n
    gated = np.frombuffer(raw, np.int32, n, o); o += 4 * n
    tier = np.frombuffer(raw, np.int32, n, o); o += 4 * n
    out = np.frombuffer(raw, np.float64, n * 3, o).reshape(n, 3)
    return blocked, gated, tier, out


def host_scene(acceler, seed=5):
    """Drones (pos, r, vel, des, cone, tc_min; the candidates from vel) and buildings with patrols on a 24 x 24 x 10 map.
    Planted, around building 0 (static, at (12, 12), h 6, r 1.5) and building 1 (static, a slab: h 9, r 3 at (5, 18)):
    drone 0 hovers over roof 0 with a candidate (0, 0, .): inside the disk with a == 0, and others that leave it or sink
    onto it; drone 1 climbs at roof 0 from outside; drone 2 stands deep inside disk 1 below its roof: every candidate
    blocked, tier 3; drone 3 flies at slab 1 from 4 m: every candidate blocked at its own time; drones 4, 5: every
    free candidate in a cone (tier 2), tc_min 0 and 0.7; drone 6: no live candidate (tier 4); drone 7: no candidate at
    all (counts 0); drone 8 hovers over roof 1 and climbs."""
    rng = np.random.default_rng(seed)
    n, nb = 96, 24
    pos = rng.uniform(0, 1, (n, 3)) * [24.0, 24.0, 10.0]
    ang, spd = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.0, 2.0, n)
    vel = np.stack([spd * np.cos(ang), spd * np.sin(ang), rng.uniform(-1, 1, n)], axis=-1)
    rad = np.round(rng.uniform(0.1, 0.4, n), 3)
    des = rng.uniform(-1.5, 1.5, (n, 3))
    bld = np.concatenate([rng.uniform(0, 24, (nb, 2)), rng.uniform(0, 12, (nb, 1)), rng.uniform(0.3, 2.0, (nb, 1))], axis=1)
    bld[0], bld[1] = [12.0, 12.0, 6.0, 1.5], [5.0, 18.0, 9.0, 3.0]
    bld[5, 2] = -np.inf   # a filler
    ends = np.zeros((nb, 2, 2))
    ends[:, 0] = bld[:, :2]
    ends[:, 1] = bld[:, :2] + rng.uniform(-6, 6, (nb, 2))
    speed = rng.uniform(0.3, 1.5, nb)
    speed[::3] = 0.0
    speed[1] = 0.0
    ends[5], speed[5] = np.nan, np.nan
    leg = np.ones(nb, np.uint8)
    ends[2, 1], speed[2] = bld[2, :2] + [0.3, 0.4], 1.0   # an arrival: d = 0.5 <= step
    pos[0], vel[0], rad[0] = [12.0, 12.0, 6.5], [0.5 if acceler == 0.5 else 0.0, 0.5 if acceler == 0.5 else 0.0, -0.5], 0.25
    pos[1], vel[1], rad[1] = [7.0, 12.0, 3.0], [1.5, 0.0, 1.0], 0.25
    pos[2], vel[2], rad[2] = [5.5, 18.5, 2.0], [0.3, 0.2, 0.0], 0.25
    pos[3], vel[3], rad[3] = [5.0, 11.0, 2.0], [0.0, 2.0, 0.0], 0.25
    pos[8], vel[8], rad[8] = [5.0, 18.0, 9.5], [vel[0][0], vel[0][1], 1.0], 0.25
    cone = rng.integers(0, 2 ** 63, n, dtype=np.uint64) & rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    cone[::4] = 0
    tc_min = rng.choice([0.0, 0.7, 3.2, np.inf], n)
    cone[4], cone[5], tc_min[4], tc_min[5] = 2 ** 64 - 1, 2 ** 64 - 1, 0.0, 0.7
    drones = np.zeros((n, 20))
    cnts, masks, cands = np.zeros((n, 3), np.int32), np.zeros((n, 2), np.uint64), []
    for i in range(n):
        vals, cnt, live = ref.candidates(vel[i], (2.0, 2.0, 1.5), acceler)
        if i == 6:
            live = 0
        if i == 7:
            vals, cnt, live = [[], [], []], [0, 0, 0], 0
        cands.append((vals, cnt))
        drones[i, :3], drones[i, 3], drones[i, 16], drones[i, 17:] = pos[i], rad[i], tc_min[i], des[i]
        for k in range(3):
            drones[i, 4 + 4 * k:4 + 4 * k + cnt[k]] = vals[k]
        cnts[i], masks[i] = cnt, [live, cone[i]]
    return drones, cnts, masks, cands, bld, (ends, speed, leg)


@pytest.mark.parametrize("acceler,moving,par", [(0.5, False, PAR), (1.0, False, PAR), (1.0, True, PAR), (0.5, True, PAR),
                                                (1.0, True, dict(PAR, clear_xy=0.4, clear_z=1.5, horizon=2.5))])
def test_host_functions_equal_the_restatement(exe, tmp_path, acceler, moving, par):
    """(b) blocked mask, n_gated, tier and out_vel of the header's functions: the restatement's bits, with every branch of
    rule 2 and every tier seen (the tally is asserted on the static scenes, where the plants are what their comment says)."""
    import building_rows_moving_ref as ref8
    drones, cnts, masks, cands, bld, motion = host_scene(acceler)
    ends, speed, leg = motion
    blocked, gated, tier, out = _run(exe, tmp_path, drones, cnts, masks, bld, motion if moving else None, 1.0, par)
    vel_of = (lambda j: ref8.velocity(bld[j], ends[j], speed[j], leg[j], 1.0)) if moving else (lambda j: (0.0, 0.0, 0))
    tally = collections.Counter()
    kw = {k: par[k] for k in ("horizon", "reach", "below", "clear_xy", "clear_z")}
    for i, d in enumerate(drones):
        vals, cnt = cands[i]
        w_blocked, w_gated, tb = ref.sweep(d[:3], d[3], vals, cnt, int(masks[i, 0]), bld, vel_of, tally=tally, **kw)
        w_tier, w_out = ref.select(vals, cnt, int(masks[i, 0]), int(masks[i, 1]), w_blocked, tb, d[16], d[17:], tally=tally)
        assert int(blocked[i]) == w_blocked, (i, hex(int(blocked[i])), hex(w_blocked))
        assert gated[i] == w_gated and tier[i] == w_tier, (i, gated[i], w_gated, tier[i], w_tier)
        assert np.array_equal(out[i].view(np.int64), np.array(w_out).view(np.int64)), (i, out[i], w_out)
    print(acceler, moving, dict(tally))
    assert (tier[4:8] == [2, 2, 4, 4]).all() and not out[6].any() and not out[7].any()
    assert tier[2] == 3 and int(blocked[2]) == int(masks[2, 0])   # inside a standing disk below its roof
    if acceler == 0.5 and not moving:   # (with four values per axis drone 3 finds a way round the slab)
        assert tier[3] == 3 and int(blocked[3]) == int(masks[3, 0])
    for name in ref.BRANCHES:
        if par is PAR:   # (with 1.5 m over the roofs the hovering drones are below H: blocked, not descending)
            assert tally[name] >= 3, (name, dict(tally))
    for t in ("tier1", "tier2", "tier3", "tier4"):
        assert tally[t] >= 2, (t, dict(tally))
    assert gated.max() >= 3 and (gated == 0).any() is not None


def test_argument_table_and_rule_two_branch_by_branch(exe):
    """The program's self-test: every refusal of rvo3d_rvo_vel_city's argument check and rule 2 on hand-computed cases."""
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    print(res.stderr)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "rvo city ok" in res.stdout


# ---- (c) ----------------------------------------------------------------------------------------------------------------------

def fly(scene, controller, steps):
    """One episode of the fixture scene through the oracle's step, as post_train.policy_test flies it: until a drone is done,
    all have finished or `steps` are flown.  controller "des": env.des_vel(); "rvo_city": the restatement with the
    scene's parameters.  Returns (minimum building clearance over the steps, steps flown, tiers seen)."""
    from rvo3d_amd.safety import safety_numpy
    wp, npts, ms, bld, rad = (scene[k] for k in ("waypoints", "n_points", "map_size", "buildings", "radius"))
    kw = {k: float(scene[k]) for k in ("acceler", "horizon", "clear_xy", "clear_z")}
    E, N = npts.shape
    assert E == 1
    env = orc.OracleEnv(wp, npts, ms, bld, nm=int(scene["nm"]))
    env.reset()
    worst, tiers = np.inf, collections.Counter()
    for t in range(steps):
        s, des = env.get_state(), env.des_vel()
        if controller == "des":
            a = des
        else:
            a = np.zeros((1, N, 3))
            for i in range(N):
                vals, cnt, live = ref.candidates(s["vel"][0, i], (2.0, 2.0, 2.0), kw["acceler"])
                cone, tc_min = ref.drone_side(i, s["pos"][0], s["vel"][0], np.full(N, float(rad)), np.ones(N), vals, cnt, live)
                blocked, _, tb = ref.sweep(s["pos"][0, i], float(rad), vals, cnt, live, bld, lambda j: (0.0, 0.0),
                                           kw["horizon"], 10.0, 1.0, kw["clear_xy"], kw["clear_z"], tally=tiers)
                tier, a[0, i] = ref.select(vals, cnt, live, cone, blocked, tb, tc_min, des[0, i], tally=tiers)
        _, _, _, done, _, fin = env.step(a)
        _, bclear, _, _ = safety_numpy(env.get_state()["pos"], float(rad), ms, 0.5, buildings=bld)
        worst = min(worst, float(bclear.min()))
        if done.any() or fin.all():
            return worst, t + 1, tiers
    return worst, steps, tiers


def test_closed_loop_keeps_clear_of_the_buildings_where_des_vel_flies_into_one():
    """(c) 1 env, 8 drones, a shared static list of buildings across the routes, at most 60 steps: following des_vel ends
    inside a building (bclear <= 0), the city controller keeps bclear > 0 on every step of its episode - and it is the
    buildings that make the difference: some candidates were blocked on the way."""
    scene = np.load(SCENE)
    assert scene["n_points"].shape == (1, 8) and 2 <= len(scene["buildings"]) <= 8 and int(scene["steps"]) <= 60
    steps = int(scene["steps"])
    d_worst, d_steps, _ = fly(scene, "des", steps)
    c_worst, c_steps, tally = fly(scene, "rvo_city", steps)
    print("des_vel: bclear", d_worst, "after", d_steps, "steps; rvo_city: bclear", c_worst, "over", c_steps, "steps", dict(tally))
    assert d_worst <= 0.0
    assert c_worst > 0.0
    assert tally["blocked"] + tally["descending_onto_roof"] > 0 and tally["tier1"] > 0
