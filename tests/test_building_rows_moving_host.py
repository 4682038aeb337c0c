"""The host-testable halves of the building rows for moving buildings (include/rvo3d.h: rvo3d_building_rows_moving), no
GPU needed:

  (a) tests/building_rows_moving_ref.py - the plain-Python restatement the GPU tests compare the kernel against - against
      tests/golden/calls_building_time_rel.npz, which tools/gen_golden_building_time_rel.py recorded from the reference's
      own cal_exp_tim_with_building at the relative velocity;
  (b) tests/host/building_rows_moving_check.hip - a stand-alone CPU program over the header's __host__ __device__ functions
      (csrc/rvo3d_building_kernels.hpp: building_row_moving; csrc/rvo3d_motion_kernels.hpp: motion_velocity) - against the
      restatement, bit for bit, on seeded scenes with every branch of the velocity rule planted;
  (c) the argument-check table with 8k, the launch geometry and the velocity rule's branches: the program's self-test.

The program is built with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and run as a child process."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import building_motion_ref as mref
import building_rows_moving_ref as ref
import building_rows_ref as ref6

CSRC = os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "building_rows_moving_check.hip")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-O1",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("building_rows_moving") / "building_rows_moving_check")
    subprocess.check_call([hipcc] + FLAGS + ["-I", CSRC, "-o", out, SRC])
    return out


def test_restatement_equals_the_reference_at_the_relative_velocity():
    """(a) The branch of t equal wherever |c| and |disc| exceed 1e-9 of their scale (zero relative velocity: scale 0,
    decided, not exempt), finite t within 1e-12 relative.  Exempt pairs are counted, printed, and at most 1 % of all.  The
    planted pairs are what they were planted for: a building aimed at a standing drone has a finite time where the static
    one is +inf, a building moving with its drone +inf where the static one is finite."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "calls_building_time_rel.npz"))
    pos, vel, rad, bld, vb, t_ref = (fx[k] for k in ("pos", "vel", "radius", "buildings", "building_vel", "t"))
    nd, nb = t_ref.shape
    assert (vb[::5] == 0).all() and vb.any(axis=1).sum() >= nb // 2 and np.hypot(vb[:, 0], vb[:, 1]).max() <= 2.0
    exempt = 0
    seen = dict(zero=0, inf=0, finite=0, zero_rel_vel=0)
    for i in range(nd):
        for j in range(nb):
            q = ref.pair(pos[i], vel[i], rad[i], bld[j], vb[j])
            ex, ey, R = pos[i, 0] - bld[j, 0], pos[i, 1] - bld[j, 1], rad[i] + bld[j, 3]
            rvx, rvy = vel[i, 0] - vb[j, 0], vel[i, 1] - vb[j, 1]
            a, bq = rvx ** 2 + rvy ** 2, 2 * ex * rvx + 2 * ey * rvy
            sure = abs(q["c"]) > 1e-9 * (ex * ex + ey * ey + R * R)
            if sure and q["branch"] != 0:
                scale = bq * bq + 4.0 * a * abs(q["c"])
                sure = abs(q["disc"]) > 1e-9 * scale or scale == 0.0
                seen["zero_rel_vel"] += scale == 0.0
            if not sure:
                exempt += 1
                continue
            tr = float(t_ref[i, j])
            if q["t_rel"] == 0.0:
                assert tr == 0.0, (i, j)
                seen["zero"] += 1
            elif np.isinf(q["t_rel"]):
                assert np.isinf(tr) and tr > 0, (i, j, tr)
                seen["inf"] += 1
            else:
                assert np.isfinite(tr) and abs(q["t_rel"] - tr) <= 1e-12 * abs(tr), (i, j, q["t_rel"], tr)
                seen["finite"] += 1
    print("pairs", nd * nb, "exempt", exempt, "seen", seen)
    assert exempt * 100 <= nd * nb
    assert min(seen.values()) > 3 and seen["zero"] > 20 and seen["finite"] > 20
    assert len(fx["aimed_pairs"]) >= 4 and len(fx["with_pairs"]) >= 4
    for i, j in fx["aimed_pairs"]:
        q = ref.pair(pos[i], vel[i], rad[i], bld[j], vb[j])
        assert not vel[i, :2].any() and np.isinf(q["t"]) and 0 < q["t_rel"] < np.inf and q["row6"][5] == 0 < q["row"][5]
    for i, j in fx["with_pairs"]:
        q = ref.pair(pos[i], vel[i], rad[i], bld[j], vb[j])
        assert 0 < q["t"] < np.inf and np.isinf(q["t_rel"]) and q["row"][5] == 0 < q["row6"][5]


def _run(exe, tmp_path, drones, bld, k, motion=None, dt=1.0, reach=5.0, below=2.0):
    drones, bld = np.ascontiguousarray(drones, dtype=np.float64), np.ascontiguousarray(bld, dtype=np.float64).reshape(-1, 4)
    n, nb = len(drones), len(bld)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, nb, k, motion is not None], dtype=np.int32).tobytes())
        f.write(np.array([reach, below, dt], dtype=np.float64).tobytes())
        f.write(drones.tobytes())
        f.write(bld.tobytes())
        if motion is not None:
            ends, speed, leg = motion
            f.write(np.ascontiguousarray(ends, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(speed, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(leg, dtype=np.uint8).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    raw = open(fout, "rb").read()
    o = 0
    cnt = np.frombuffer(raw, np.int32, n, o); o += 4 * n
    rows = np.frombuffer(raw, np.float32, n * k * 8, o).reshape(n, k, 8); o += 4 * n * k * 8
    vb = np.frombuffer(raw, np.float64, nb * 2, o).reshape(nb, 2)
    return cnt, rows, vb


# the planted records of scene(): (index, what)
STATIC, NAN_SPEED, ON_ENDPOINT, D_EQ_STEP, D_ABOVE_STEP, FILLER = 0, 1, 2, 3, 4, 5


def scene(dt):
    """The fixture's drones and buildings; patrols with endpoint 1 within 6 m and speeds 0.3 .. 1.5, every fourth speed 0;
    the records 0..5 planted (dt = 1 in mind): speed 0, a NaN speed, a record standing on the endpoint it approaches
    (d == 0), one whose endpoint is exactly one step away ((3, 4) at speed 5: d == step), the same a hair slower (d just
    above step), and a filler (h = -inf, NaN ends and speed: never read).  Two moves bring some records onto leg 0."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "calls_building_time_rel.npz"))
    drones = np.concatenate([fx["pos"], fx["vel"][:, :2], fx["radius"][:, None]], axis=1)
    bld = fx["buildings"].copy()
    nb = len(bld)
    rng = np.random.default_rng(77)
    r, a = 6.0 * np.sqrt(rng.uniform(0, 1, nb)), rng.uniform(0, 2 * np.pi, nb)
    ends = np.zeros((nb, 2, 2))
    ends[:, 0] = bld[:, :2]
    ends[:, 1, 0], ends[:, 1, 1] = bld[:, 0] + r * np.cos(a), bld[:, 1] + r * np.sin(a)
    speed = rng.uniform(0.3, 1.5, nb)
    speed[8::4] = 0.0
    leg = np.ones(nb, np.uint8)
    if dt > 0:   # two moves: positions off the endpoints, some arrivals (leg 0)
        b, l = bld[None], leg[None]
        for _ in range(2):
            b, l = mref.move(b, ends[None], speed[None], l, dt)
        bld, leg = b[0].copy(), l[0].copy()
    speed[STATIC] = 0.0
    speed[NAN_SPEED] = np.nan
    ends[ON_ENDPOINT, 1], speed[ON_ENDPOINT], leg[ON_ENDPOINT] = bld[ON_ENDPOINT, :2], 1.0, 1
    bld[D_EQ_STEP, :2] = [20.0, 30.0]
    ends[D_EQ_STEP, 1], speed[D_EQ_STEP], leg[D_EQ_STEP] = [23.0, 34.0], 5.0, 1
    bld[D_ABOVE_STEP, :2] = [12.0, 9.0]
    ends[D_ABOVE_STEP, 1], speed[D_ABOVE_STEP], leg[D_ABOVE_STEP] = [15.0, 13.0], np.nextafter(5.0, 0.0), 1
    bld[FILLER, 2] = -np.inf
    ends[FILLER], speed[FILLER] = np.nan, np.nan
    # a drone next to each planted record, so that it is kept in somebody's rows
    for b in (STATIC, NAN_SPEED, ON_ENDPOINT, D_EQ_STEP, D_ABOVE_STEP):
        drones[b, :3] = [bld[b, 0] + bld[b, 3] + 0.7, bld[b, 1] + 0.1, min(bld[b, 2], 3.0)]
    return drones, bld, (ends, speed, leg)


@pytest.mark.parametrize("k,dt", [(1, 1.0), (3, 1.0), (8, 1.0), (3, 0.5), (3, 0.0)])
def test_host_functions_equal_the_restatement(exe, tmp_path, k, dt):
    """(b) Rows, counts and the velocities of the header's functions: the restatement's bits - with every branch of the
    velocity rule among the kept rows, and columns 0..4 those of the rows of six."""
    drones, bld, motion = scene(dt)
    ends, speed, leg = motion
    cnt, rows, vb = _run(exe, tmp_path, drones, bld, k, motion, dt)
    branch = np.zeros(len(bld), np.int64)
    for j, b in enumerate(bld):
        if b[2] == -np.inf:
            assert not vb[j].any()
            continue
        vx, vy, branch[j] = ref.velocity(b, ends[j], speed[j], leg[j], dt)
        assert np.array_equal(vb[j].view(np.int64), np.array([vx, vy]).view(np.int64)), (j, vb[j], vx, vy)
    if dt == 1.0:
        assert (branch[[STATIC, NAN_SPEED]] == 0).all() and (branch[[ON_ENDPOINT, D_EQ_STEP]] == 1).all()
        assert branch[D_ABOVE_STEP] == 2 and not vb[ON_ENDPOINT].any() and vb[D_EQ_STEP].tolist() == [3.0, 4.0]
        assert 0 < 5.0 - np.hypot(*vb[D_ABOVE_STEP]) < 1e-14
    if dt == 0.0:
        assert not vb.any() and not branch.any()
    kept_branches, differs = set(), 0
    vel_of = lambda j: ref.velocity(bld[j], ends[j], speed[j], leg[j], dt)
    for i, d in enumerate(drones):
        p, v, r = d[:3], (d[3], d[4], 0.0), d[5]
        w_rows, w_cnt, kept, info = ref.drone_rows(p, v, r, bld, k, vel_of)
        assert cnt[i] == w_cnt, i
        assert np.array_equal(rows[i].view(np.int32), w_rows.view(np.int32)), (i, rows[i], w_rows)
        assert not (np.signbit(rows[i]) & (rows[i] == 0)).any()   # no -0.0
        rows6, cnt6, kept6 = ref6.drone_rows(p, v, r, bld, k)
        assert kept == kept6 and cnt6 == w_cnt and FILLER not in kept
        assert np.array_equal(rows[i][:, :5].view(np.int32), rows6[:, :5].view(np.int32)), i
        for s, q in enumerate(info):
            kept_branches.add(q["branch"])
            differs += bool(q["urg6"] != q["urg8"])
            if q["branch"] == 0:   # a static record inside a moving set: the row of six and two zeros
                assert np.array_equal(rows[i][s, :6].view(np.int32), rows6[s].view(np.int32)) and not rows[i][s, 6:].any()
    if dt == 0.0:
        assert kept_branches == {0} and differs == 0
    else:
        assert kept_branches == {0, 1, 2} and differs > 0, (kept_branches, differs)
    if k == 8 and dt == 1.0:
        for b in (STATIC, NAN_SPEED, ON_ENDPOINT, D_EQ_STEP, D_ABOVE_STEP):   # the planted records are in their drone's rows
            assert b in ref6.drone_rows(drones[b][:3], (drones[b][3], drones[b][4], 0.0), drones[b][5], bld, k)[2], b


@pytest.mark.parametrize("k", [1, 4])
def test_without_a_motion_the_rows_are_the_six_floats_and_two_zeros(exe, tmp_path, k):
    """Rule 5."""
    drones, bld, _ = scene(1.0)
    cnt, rows, vb = _run(exe, tmp_path, drones, bld, k, None)
    assert not vb.any()
    some = 0
    for i, d in enumerate(drones):
        rows6, cnt6, _ = ref6.drone_rows(d[:3], (d[3], d[4], 0.0), d[5], bld, k)
        assert cnt[i] == cnt6
        assert np.array_equal(rows[i][:, :6].view(np.int32), rows6.view(np.int32)), i
        assert not rows[i][:, 6:].view(np.int32).any(), i   # +0.0: no bit set
        w_rows, _, _, _ = ref.drone_rows(d[:3], (d[3], d[4], 0.0), d[5], bld, k, lambda j: (0.0, 0.0, 0))
        assert np.array_equal(rows[i].view(np.int32), w_rows.view(np.int32)), i
        some += int(cnt6 > 0)
    assert some > 50


def test_argument_table_geometry_and_velocity_branches(exe):
    """(c) the program's self-test: every refusal of rvo3d_building_rows_moving's argument check (8k; the motion; dt), the
    LDS budget of every fleet size and k, the velocity rule branch by branch and next to motion_move."""
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    print(res.stderr)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "building rows moving ok" in res.stdout


def test_scenes_of_the_gpu_module():
    """tests/test_gpu_building_rows_moving.py's host-side scene: its shapes, its plants and the non-vacuity counts of its
    docstring, recounted here from the restatement (no GPU)."""
    import test_gpu_building_rows_moving as g
    assert set(g.TALLY_K3) == set(g.TALLY_K1) == set(g.SHAPES)
    for k, table in ((3, g.TALLY_K3), (1, g.TALLY_K1)):
        for shape, want in table.items():
            sc = g.moved_scene(*shape)
            _, _, tally, _ = ref.building_rows_moving_ref(sc.pos, sc.vel, sc.rad, sc.bld, k, (sc.ends, sc.speed, sc.leg), g.DT,
                                                       building_counts=sc.cnt)
            got = tuple(int(tally[n]) for n in g.TALLY_NAMES)
            print(shape, "k", k, got)
            assert got == want and min(got if k == 3 else got[:4]) >= 1, (shape, k, got, want)
