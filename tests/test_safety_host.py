"""The host-testable halves of the safety metrics (include/rvo3d.h: rvo3d_safety_scan, rvo3d_eval_account_safety), no GPU
needed:

  * rvo3d_amd.safety.safety_numpy - the numpy restatement the GPU tests compare the kernel against - on a case worked out
    by hand, and under a permutation of the drones;
  * the episode fold the account kernel runs (csrc/rvo3d_safety_kernels.hpp: eval_safety_fold / eval_safety_keep behind
    eval_account_env) - tests/host/safety_account_check.hip is a stand-alone program that calls it and no HIP function,
    built here with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and run as a child process;
  * the three predicates against the C oracle's `done` on a world with buildings;
  * summarize_safety on records written out by hand."""
import os
import shutil
import subprocess

import numpy as np

from conftest import ROOT
from golden_util import load

CSRC = os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "safety_account_check.hip")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-O1",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
INF = np.inf


def test_hand_case():
    """Three drones of radius 0.25 and one building (4, 4, h = 1, r = 0.5) in a 10 x 10 x 5 map:
      d0 (0, 1, 1)        on the face x = 0, at p_z == h: the building counts, d = sqrt(16 + 9) = 5;
      d1 (0, 1, 1.5)      0.5 above d0: dis == r_0 + r_1 exactly; above the building;
      d2 (-2^-30, 5, 1+)  just outside the face x = 0, at nextafter(h, inf): the building does not count; from d0
                          rel = (2^-30, -4, -2^-52), (16 + 2^-60) + 2^-104 rounds to 16: dis = 4; from d1 the sum rounds
                          to 16.25, dis - 0.5 = 3.53..."""
    from rvo3d_amd.safety import safety_numpy
    z2 = np.nextafter(1.0, INF)
    pos = np.array([[[0.0, 1.0, 1.0], [0.0, 1.0, 1.5], [-2.0 ** -30, 5.0, z2]]])
    bld = np.array([[4.0, 4.0, 1.0, 0.5]])
    sep, bclear, wall, near = safety_numpy(pos, 0.25, (10.0, 10.0, 5.0), 0.5, buildings=bld)
    assert sep.tolist() == [[0.0, 0.0, 3.5]]
    assert bclear.tolist() == [[4.25, INF, INF]]
    assert wall.tolist() == [[0.0, 0.0, -2.0 ** -30]]
    assert not np.signbit(wall[0, :2]).any()
    assert near.tolist() == [1] and near.dtype == np.int32
    # the predicates of `done`: sep <= 0 (d0, d1), bclear <= 0 (nobody), wall < 0 (d2 alone: on the face is inside)
    assert ((sep <= 0) | (bclear <= 0) | (wall < 0)).tolist() == [[True, True, True]]
    assert (wall < 0).tolist() == [[False, False, True]]
    # near_margin is inclusive, and colliding pairs count
    assert safety_numpy(pos, 0.25, (10.0, 10.0, 5.0), 3.5, buildings=bld)[3].tolist() == [2]
    assert safety_numpy(pos, 0.25, (10.0, 10.0, 5.0), 0.0, buildings=bld)[3].tolist() == [1]
    # the same list as a per-env set, with an unused record behind it; then with the count cut to 0
    env_b = np.array([[[4.0, 4.0, 1.0, 0.5], [0.0, 1.0, 9.0, 9.0]]])
    assert safety_numpy(pos, 0.25, (10.0, 10.0, 5.0), 0.5, buildings=env_b, building_counts=[1])[1].tolist() == \
        [[4.25, INF, INF]]
    assert safety_numpy(pos, 0.25, (10.0, 10.0, 5.0), 0.5, buildings=env_b, building_counts=[0])[1].tolist() == \
        [[INF, INF, INF]]
    assert safety_numpy(pos, 0.25, (10.0, 10.0, 5.0), 0.5, buildings=env_b)[1][0, 0] == -9.25   # inside the second
    # counts: the third row is a ghost (never read: NaN there changes nothing), its outputs are +inf
    ghost = pos.copy()
    ghost[0, 2] = np.nan
    s2, b2, w2, n2 = safety_numpy(ghost, 0.25, (10.0, 10.0, 5.0), 4.0, counts=[2], buildings=bld)
    assert s2.tolist() == [[0.0, 0.0, INF]] and b2.tolist() == [[4.25, INF, INF]] and w2.tolist() == [[0.0, 0.0, INF]]
    assert n2.tolist() == [1]
    # a sole drone has no separation
    s1, _, w1, n1 = safety_numpy(pos[:, :1], 0.25, (10.0, 10.0, 5.0), 0.5)
    assert s1.tolist() == [[INF]] and w1.tolist() == [[0.0]] and n1.tolist() == [0]


def test_order_independence():
    """Permuting the drones permutes the rows and changes nothing else - bit for bit, with pairs at equal distances and
    drones at equal positions among them."""
    from rvo3d_amd.safety import safety_numpy
    rng = np.random.default_rng(11)
    E, N = 3, 17
    ms = np.array([12.0, 9.0, 6.0])
    pos = rng.uniform(-0.2, 1.0, (E, N, 3)) * ms
    pos[:, 5] = pos[:, 2]                       # a shared position
    pos[:, 7] = pos[:, 2] + [0.4, 0.0, 0.0]      # ties
    pos[:, 8] = pos[:, 2] - [0.4, 0.0, 0.0]
    rad = rng.uniform(0.1, 0.4, (E, N))
    bld = np.concatenate([rng.uniform(1, 8, (E, 6, 2)), rng.uniform(0, 6, (E, 6, 1)), rng.uniform(0.5, 1.5, (E, 6, 1))], axis=2)
    cnt = np.array([6, 0, 3])
    want = safety_numpy(pos, rad, ms, 0.5, buildings=bld, building_counts=cnt)
    assert np.isfinite(want[1][0]).any() and np.isinf(want[1][1]).all() and (want[3] > 0).any()
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(N)
        got = safety_numpy(pos[:, perm], rad[:, perm], ms, 0.5, buildings=bld, building_counts=cnt)
        for k in range(3):
            assert np.array_equal(got[k].view(np.int64), want[k][:, perm].view(np.int64)), k
        assert np.array_equal(got[3], want[3])
    # the buildings' order does not show either
    bperm = np.random.default_rng(9).permutation(6)
    got = safety_numpy(pos[:1], rad[:1], ms, 0.5, buildings=bld[:1, bperm])
    assert np.array_equal(got[1].view(np.int64), safety_numpy(pos[:1], rad[:1], ms, 0.5, buildings=bld[:1])[1].view(np.int64))


def test_episode_fold_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "safety_account_check")
    subprocess.check_call([hipcc] + FLAGS + ["-I", CSRC, "-o", exe, SRC])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout)
    print(res.stderr)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "safety account ok" in res.stdout


def excluded_rows(pos, radius, buildings, n=None):
    """The rows the cross-check against `done` may leave out, [N] bool: drones that share their exact position with
    another drone (quirk Q6: the reference excludes itself from its neighbours by position, so such a pair never
    collides there) and drones for which a building's r_i + r_b exceeds the reference's 5 m gate."""
    n = pos.shape[0] if n is None else n
    p = pos[:n]
    same = (p[:, None, :] == p[None, :, :]).all(axis=2) & ~np.eye(n, dtype=bool)
    out = np.zeros(pos.shape[0], dtype=bool)
    out[:n] = same.any(axis=1)
    if len(buildings):
        out[:n] |= ((np.asarray(radius)[:n, None] + np.asarray(buildings)[None, :, 3]) > 5.0).any(axis=1)
    return out


def test_predicates_equal_the_oracles_done():
    """The C oracle (env_train = 1) steps tests/golden/scatter3_n32_nm10.npz - 32 drones, 5 buildings, the fixture's own
    actions, drones with done | finish reset behind each step as the trainer does -; after every step, for every drone,
    done == (sep <= 0 or bclear <= 0 or wall < 0) on the state the step left.  On this fixture no row is left out."""
    import oracle
    from rvo3d_amd.safety import safety_numpy
    fx = load(os.path.join(ROOT, "tests", "golden", "scatter3_n32_nm10.npz"))
    assert int(fx["env_train"]) == 1 and fx["buildings"].shape[0] > 0
    N = fx["waypoints"].shape[0]
    rad = np.full((1, N), float(fx["radius"]))
    env = oracle.OracleEnv(fx["waypoints"][None], fx["n_points"][None], fx["map_size"], fx["buildings"],
                           nm=int(fx["nm"]), env_train=True, radius=rad)
    rows = left_out = 0
    fired = np.zeros(3, dtype=np.int64)
    for a in fx["actions"]:
        _, _, _, done, _, fin = env.step(a[None])
        pos = env.get_state()["pos"]
        sep, bclear, wall, _ = safety_numpy(pos, rad, fx["map_size"], 0.5, buildings=fx["buildings"])
        keep = ~excluded_rows(pos[0], rad[0], fx["buildings"])
        pred = (sep[0] <= 0) | (bclear[0] <= 0) | (wall[0] < 0)
        assert np.array_equal(done[0].astype(bool)[keep], pred[keep])
        rows += N
        left_out += int((~keep).sum())
        fired += [int((sep <= 0).sum()), int((bclear <= 0).sum()), int((wall < 0).sum())]
        env.reset_drones((done | fin)[0])
    print("rows", rows, "left out", left_out, "fired: pairs, buildings, walls", fired.tolist())
    assert left_out * 100 <= rows and left_out == 0
    assert (fired > 0).all()   # each of the three predicates was seen true


def test_summary_of_records():
    from rvo3d_amd.safety import summarize_safety
    s = summarize_safety(min_sep=[0.5, -0.1, INF, 1.5], min_bclear=[INF] * 4, min_wall=[1.0, 2.0, 0.0, 1.0],
                         near=[0, 3, 0, 1], length=[10, 20, 30, 40], drones=[4, 4, 1, 2])
    assert s["episodes"] == 4
    assert s["mean_min_sep"] == (0.5 - 0.1 + 1.5) / 3 and s["min_min_sep"] == -0.1     # (+inf: no second drone)
    assert np.isnan(s["mean_min_bclear"]) and s["min_min_bclear"] == INF                # no building ever counted
    assert s["mean_min_wall"] == 1.0 and s["min_min_wall"] == 0.0
    assert s["near_per_1000_drone_steps"] == 1000.0 * 4 / (40 + 80 + 30 + 80)
    assert s["near_episode_share"] == 0.5
    # one drone count for every episode, records as the device leaves them ([E][quota])
    s2 = summarize_safety(np.array([[1.0, 2.0]]), np.array([[3.0, 1.0]]), np.array([[0.5, 0.25]]), np.array([[2, 0]]),
                          np.array([5, 5]), 8)
    assert s2["mean_min_sep"] == 1.5 and s2["min_min_bclear"] == 1.0 and s2["near_per_1000_drone_steps"] == 25.0
