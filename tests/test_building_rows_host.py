"""The host-testable halves of the nearest-building rows (include/rvo3d.h: rvo3d_building_rows), no GPU needed:

  (a) tests/building_rows_ref.py - the plain-Python restatement the GPU tests compare the kernel against - against
      tests/golden/calls_building_rows.npz, which tools/gen_golden_building_rows.py recorded from the reference's own
      rvo_inter.preprocess and cal_exp_tim_with_building;
  (b) tests/host/building_rows_check.hip - a stand-alone CPU program over the header's __host__ __device__ row and
      insertion functions (csrc/rvo3d_building_kernels.hpp) - against the restatement, bit for bit;
  (c) the argument-check table (building_rows_check, a pure function) and the launch geometry: the program's self-test."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import building_rows_ref as ref

CSRC = os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "building_rows_check.hip")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-O1"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("building_rows") / "building_rows_check")
    subprocess.check_call([hipcc] + FLAGS + ["-I", CSRC, "-o", out, SRC])
    return out


def test_restatement_equals_the_reference():
    """(a) Gate decisions equal for every pair further than 1e-9 from both thresholds - and for the exact cases (offset
    (3, 4): d == 5.0 passes; h_b == p_z - 2 fails) without exemption; the branch of t equal wherever |c| and |disc| exceed
    1e-9 of their scale, finite t within 1e-12 relative (the reference's ** 2 goes through pow).  Exempt pairs are counted,
    printed, and at most 1 % of all."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "calls_building_rows.npz"))
    pos, vel, rad, bld, kept, t_ref = (fx[k] for k in ("pos", "vel", "radius", "buildings", "kept", "t"))
    nd, nb = kept.shape
    exact = {tuple(x) for x in fx["exact_pairs"].tolist()}
    assert (0, 0) in exact and kept[0, 0] and (2, 1) in exact and not kept[2, 1]
    exempt_gate = exempt_t = 0
    seen = dict(zero=0, inf=0, finite=0)
    for i in range(nd):
        for j in range(nb):
            q = ref.pair(pos[i], vel[i], rad[i], bld[j])
            if (i, j) in exact:
                assert q["passes"] == bool(kept[i, j]), (i, j)
            elif abs(q["d"] - 5.0) > 1e-9 and abs(bld[j, 2] - (pos[i, 2] - 2.0)) > 1e-9:
                assert q["passes"] == bool(kept[i, j]), (i, j, q["d"])
            else:
                exempt_gate += 1
            ex, ey, R = pos[i, 0] - bld[j, 0], pos[i, 1] - bld[j, 1], rad[i] + bld[j, 3]
            a, bq = vel[i, 0] ** 2 + vel[i, 1] ** 2, 2 * ex * vel[i, 0] + 2 * ey * vel[i, 1]
            c_scale = ex * ex + ey * ey + R * R
            sure = abs(q["c"]) > 1e-9 * c_scale
            if sure and q["branch"] != 0:
                # (a drone that stands still has a == bq == 0 exactly on both sides - 0 ** 2 and 2 * x * 0 are exact -, so
                # disc == 0 is no rounding accident there: scale 0 is sure)
                scale = bq * bq + 4.0 * a * abs(q["c"])
                sure = abs(q["disc"]) > 1e-9 * scale or scale == 0.0
            if not sure:
                exempt_t += 1
                continue
            tr = float(t_ref[i, j])
            if q["t"] == 0.0:
                assert tr == 0.0, (i, j)
                seen["zero"] += 1
            elif np.isinf(q["t"]):
                assert np.isinf(tr) and tr > 0, (i, j, tr)
                seen["inf"] += 1
            else:
                assert np.isfinite(tr) and abs(q["t"] - tr) <= 1e-12 * abs(tr), (i, j, q["t"], tr)
                seen["finite"] += 1
    print("pairs", nd * nb, "exempt: gate", exempt_gate, "t", exempt_t, "seen", seen)
    assert (exempt_gate + exempt_t) * 100 <= nd * nb
    assert min(seen.values()) > 20


def _run(exe, tmp_path, drones, bld, k, reach=5.0, below=2.0):
    drones, bld = np.ascontiguousarray(drones, dtype=np.float64), np.ascontiguousarray(bld, dtype=np.float64).reshape(-1, 4)
    n, nb = len(drones), len(bld)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, nb, k], dtype=np.int32).tobytes())
        f.write(np.array([reach, below], dtype=np.float64).tobytes())
        f.write(drones.tobytes())
        f.write(bld.tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    raw = open(fout, "rb").read()
    o = 0
    cnt = np.frombuffer(raw, np.int32, n, o); o += 4 * n
    rows = np.frombuffer(raw, np.float32, n * k * 6, o).reshape(n, k, 6); o += 4 * n * k * 6
    pairs = np.frombuffer(raw, np.float64, n * nb * 3, o).reshape(n, nb, 3); o += 8 * n * nb * 3
    passes = np.frombuffer(raw, np.uint8, n * nb, o).reshape(n, nb)
    return cnt, rows, pairs, passes


def _scene():
    """The fixture's inputs (continuous coordinates, drones inside cylinders, stationary drones, the exact gate cases) and
    a hand-made corner: a drone with nine buildings in reach, two of them at equal gap, one touching exactly."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "calls_building_rows.npz"))
    drones = np.concatenate([fx["pos"], fx["vel"][:, :2], fx["radius"][:, None]], axis=1)
    bld = fx["buildings"].copy()
    ring = np.array([[50.0 + 3.0, 50.0, 9.0, 1.0], [50.0 - 3.0, 50.0, 9.0, 1.0],      # equal gaps (1.75): index decides
                     [50.0, 50.0 + 1.25, 9.0, 1.0], [50.0, 50.0 - 4.0, 9.0, 0.5],      # touching: gap 0, c == 0 -> t = 0
                     [50.0 + 2.0, 50.0 + 2.0, 9.0, 0.25], [50.0 - 1.0, 50.0 - 1.0, 9.0, 0.25],
                     [50.0 + 4.0, 50.0 - 3.0, 9.0, 2.0], [50.0 - 4.0, 50.0 + 3.0, 0.5, 2.0],  # d == 5; the last below: fails
                     [50.0, 50.0 + 4.5, 9.0, 0.125], [50.0 + 0.5, 50.0, 9.0, 0.125], [50.0 + 4.75, 50.0, 9.0, 0.125]])
    bld = np.concatenate([bld, ring])
    extra = np.array([[50.0, 50.0, 3.0, 0.5, 0.25, 0.25], [50.0, 50.0, 3.0, 0.0, 0.0, 0.25],
                      [50.0, 50.0, 3.0, -2.0, 1.0, 0.25]])
    return np.concatenate([drones, extra]), bld


@pytest.mark.parametrize("k", [1, 4, 8])
def test_host_functions_equal_the_restatement(exe, tmp_path, k):
    """(b) Rows, counts, gate decisions and the unrounded d / gap / t of the header's functions: the restatement's bits."""
    drones, bld = _scene()
    cnt, rows, pairs, passes = _run(exe, tmp_path, drones, bld, k)
    more = fewer = 0
    for i, d in enumerate(drones):
        p, v, r = d[:3], (d[3], d[4], 0.0), d[5]
        w_rows, w_cnt, _ = ref.drone_rows(p, v, r, bld, k)
        assert cnt[i] == w_cnt, i
        assert np.array_equal(rows[i].view(np.int32), w_rows.view(np.int32)), (i, rows[i], w_rows)
        assert not np.signbit(rows[i]).any() or (rows[i][np.signbit(rows[i])] != 0).all()   # no -0.0
        n_pass = 0
        for j, b in enumerate(bld):
            q = ref.pair(p, v, r, b)
            assert bool(passes[i, j]) == q["passes"], (i, j)
            got = pairs[i, j]
            want = np.array([q["d"], q["gap"], q["t"]])
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), (i, j, got, want)
            n_pass += q["passes"]
        more += n_pass > k
        fewer += 0 < n_pass < k
    assert more > 0 and (fewer > 0 or k == 1)
    # the corner drone: ten of the ring pass (one is too low); equal gaps in index order
    i = len(drones) - 3
    nb0 = len(bld) - 11
    _, _, kept = ref.drone_rows(drones[i][:3], (drones[i][3], drones[i][4], 0.0), drones[i][5], bld, 8)
    assert passes[i, nb0:].sum() == 10 and not passes[i, nb0 + 7]
    assert kept.index(nb0) + 1 == kept.index(nb0 + 1)
    if k == 8:
        assert rows[i][:, 5].max() == 5.0   # inside / touching a cylinder: urg = 5
        assert (rows[i + 1][:, 5] == 0).sum() >= 7   # the stationary drone: urg 0 but where it touches


def test_other_gates(exe, tmp_path):
    """reach and below are arguments, not constants."""
    drones, bld = _scene()
    for reach, below in ((2.5, 0.0), (40.0, 11.0)):
        cnt, rows, _, _ = _run(exe, tmp_path, drones[::7], bld, 4, reach, below)
        for i, d in enumerate(drones[::7]):
            w_rows, w_cnt, _ = ref.drone_rows(d[:3], (d[3], d[4], 0.0), d[5], bld, 4, reach, below)
            assert cnt[i] == w_cnt and np.array_equal(rows[i].view(np.int32), w_rows.view(np.int32)), (i, reach)


def test_argument_table_and_geometry(exe):
    """(c) the program's self-test: every refusal of rvo3d_building_rows's argument check, the LDS budget of every fleet
    size and k, the slot order."""
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    print(res.stderr)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "building rows ok" in res.stdout


def test_scenes_of_the_gpu_module():
    """tests/test_gpu_building_rows.py's host-side helpers: the scene cut down to fleets of one and two, and the 129-record
    list of the tile-boundary test."""
    import test_gpu_building_rows as g
    pos5, vel5, rad5, bld5, _ = g.scene(5, 5, "shared", seed=1)
    for n in (1, 2, 4):
        pos, vel, rad, bld, cnt = g.scene_cut(5, n, "shared", seed=1)
        assert pos.shape == (5, n, 3) and vel.shape == (5, n, 3) and rad.shape == (5, n) and cnt is None
        assert np.array_equal(pos, pos5[:, :n]) and np.array_equal(vel, vel5[:, :n]) and np.array_equal(bld, bld5)
    a, b = g.scene_cut(3, 7, "shared", seed=2), g.scene(3, 7, "shared", seed=2)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))
    full = g.boundary_list()
    assert full.shape == (129, 4) and np.array_equal(full, g.boundary_list()) and np.array_equal(full[:3], bld5[:3])
