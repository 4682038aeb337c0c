"""Stage X1 on the wave's compacted pair list (one-wave workgroups: x1_queue, csrc/rvo3d_pairs.hpp) and the
zero-action form of its arithmetic: a few fused auto-reset steps against the oracle, with the parity tests' own
comparison (bit-exact flags and counts, f32-exact observations and rewards, knife-edge accounting, the state on
file against the oracle's at the end) - on worlds chosen for the paths the pair list adds:

  (a) the sparse synthetic map: the list path, last trips partly filled;
  (b) every drone in range of every other: the list overflows, the per-lane loop runs;
  (c) envs whose in-range pair count is the list's capacity C - 1, C, C + 1 (and one full trip, 128 +- 1);
  (d) the crossing scene with nm = 2: kept rows truncated, requests in both directions;
  (e) envs that reset a drone next to envs that do not, in one launch: both forms of the X1 arithmetic, and
      mixed envs inside one wave at 16 / 32 drones.
"""
import numpy as np
import pytest

import oracle as orc
from rvo3d_amd import BatchedDroneEnv, World, crossing_world, synthetic_actions, synthetic_world
from test_gpu_parity import run_vs_oracle

pytestmark = pytest.mark.gpu

X1_QUEUE = 384  # kX1Queue (csrc/rvo3d_lds.hpp)
# 64 / 32 / 16 drones: one, two, four envs per wave; 48: the padded 64-drone kernel (ghost lanes own no pairs)
SHAPES = [(64, 8), (32, 8), (16, 8), (48, 4)]
KERNELS = {64: "1, 64, {t}, false>", 32: "1, 32, {t}, false>", 16: "1, 16, {t}, false>", 48: "1, 64, {t}, true>"}
SEED = 4321


def _check_kernel(world, N, env_train):
    env = BatchedDroneEnv(world, env_train=env_train)
    name = env.kernel_name("step_autoreset")
    env.close()
    assert name.endswith(KERNELS[N].format(t="true" if env_train else "false")), name


def pairs_in_range(pos, lim=10.0, clear=0.05):
    """In-range pairs of one env ([N, 3]); no pair may sit within `clear` of the 10 m gate (the fp32 stage G and
    the exact gate then agree on every pair, so the count is the length of the pair list)."""
    d = np.linalg.norm(pos[:, None] - pos[None], axis=-1)[np.triu_indices(len(pos), 1)]
    assert not ((d > lim - clear) & (d < lim + clear)).any()
    return int((d <= lim).sum())


@pytest.mark.parametrize("env_train", [True, False])
@pytest.mark.parametrize("N,E", SHAPES)
def test_sparse_map(N, E, env_train):
    """(a) 50 x 50 x 10: two to three candidates per lane, a handful of trips, the last one partly filled."""
    world = synthetic_world(E, N, (50, 50, 10))
    _check_kernel(world, N, env_train)
    st = run_vs_oracle(world, T=6, env_train=env_train, seed=SEED, name=f"x1/sparse_{N}x{E}_t{int(env_train)}")
    assert st["resets"] > 0, st


@pytest.mark.parametrize("env_train", [True, False])
@pytest.mark.parametrize("N,E", SHAPES)
def test_everybody_in_range(N, E, env_train):
    """(b) 8 x 8 x 4: all N (N - 1) / 2 pairs of an env are candidates.  64 and 48 drones (2016 / 1128 pairs) and
    four envs of 16 (480) overflow the list; two envs of 32 need more than 384 as well (992).  Nearly every env
    resets somebody in every step there and is observed at rest, so few rows are kept at all: the world's seed is
    one with which the oracle keeps some at each of the shapes and in both modes."""
    world = synthetic_world(E, N, (8, 8, 4), min_sep=0.5, seed=2)
    for e in range(E):
        assert pairs_in_range(world.waypoints[e, :, 0]) == N * (N - 1) // 2
    assert (64 // (64 if N == 48 else N)) * N * (N - 1) // 2 > X1_QUEUE
    st = run_vs_oracle(world, T=5, env_train=env_train, seed=SEED, name=f"x1/dense_{N}x{E}_t{int(env_train)}")
    assert st["resets"] > 0 and st["vo_rows"] > 0, st


def _lineup_env(n_pairs_wanted, N=64, pitch=14.0):
    """Start positions of one env with exactly n_pairs_wanted pairs in range: a block of parallel lines along +x
    (1 m apart, every drone in range of every other) and, at least 13 m from everything else, couples (1 m apart:
    one pair each) and singles."""
    m = 2
    while (m + 1) * m // 2 <= n_pairs_wanted:
        m += 1
    couples = n_pairs_wanted - m * (m - 1) // 2
    singles = N - m - 2 * couples
    assert singles >= 0 and m <= 35  # (a block of 7 x 5: diagonal 7.2 m)
    pos = [(2.0 + (k % 7), 2.0 + (k // 7), 3.0) for k in range(m)]
    for u in range(couples + singles):
        x, y = 2.0 + pitch * (u % 8), 20.0 + pitch * (u // 8)
        pos.append((x, y, 3.0))
        if u < couples:
            pos.append((x + 1.0, y, 3.0))
    return np.array(pos)


@pytest.mark.parametrize("env_train", [True, False])
def test_pair_counts_around_the_capacity(env_train):
    """(c) 64 drones, one env per wave, C - 1 / C / C + 1 pairs in range (and 127 / 128 / 129: one full trip).
    The count is that of observe() and of step 0's rows sweep, the first with velocities: a step moves nobody more
    than 1 m there (speed <= 1), a drone that resets returns to its start, so the block stays within 10 m and
    everything else more than 10 m apart.  Later steps drift from it."""
    counts = [X1_QUEUE - 1, X1_QUEUE, X1_QUEUE + 1, 127, 128, 129]
    E, N = len(counts), 64
    wp = np.empty((E, N, 2, 3))
    rng = np.random.default_rng(9)
    for e, c in enumerate(counts):
        start = _lineup_env(c)[rng.permutation(N)]  # (owners and offsets all over the ring)
        assert pairs_in_range(start) == c
        wp[e, :, 0] = start
        wp[e, :, 1] = start + np.array([30.0, 0.0, 0.0])
    world = World(wp, np.full((E, N), 2, np.int32), np.array([140.0, 110.0, 10.0]))
    _check_kernel(world, N, env_train)
    st = run_vs_oracle(world, T=4, env_train=env_train, seed=SEED, name=f"x1/capacity_t{int(env_train)}")
    assert st["vo_rows"] > 0, st


@pytest.mark.parametrize("N,E", SHAPES)
def test_crossing_nm2(N, E):
    """(d) everybody flies at the centre of the ring: requests in both directions of most pairs, more flagged
    pairs than the two rows a drone keeps."""
    world = crossing_world(E, N, (30.0, 30.0, 8.0), radius=6.0 if N > 16 else 4.0, min_sep=0.5)
    st = run_vs_oracle(world, T=6, nm=2, seed=SEED, name=f"x1/crossing_{N}x{E}")
    assert st["vo_rows"] > 0, st


def _mixed_world(E, N):
    """Even envs: crowded (9 x 9 x 4 corner of the map, somebody resets every step).  Odd envs: a 4 m grid flying
    +y, 20 m from its destinations: in range of its neighbours, nobody resets for a couple of steps."""
    world = synthetic_world(E, N, (9.0, 9.0, 4.0), min_sep=0.5, seed=SEED)
    wp = world.waypoints.copy()
    side = int(np.ceil(np.sqrt(N)))
    grid = np.array([(2.0 + 4.0 * (k % side), 2.0 + 4.0 * (k // side), 5.0) for k in range(N)])
    for e in range(1, E, 2):
        wp[e, :, 0] = grid
        wp[e, :, 1] = grid + np.array([0.0, 20.0, 0.0])
    return World(wp, world.n_points, np.array([40.0, 60.0, 10.0]))


@pytest.mark.parametrize("env_train", [True, False])
@pytest.mark.parametrize("N,E", SHAPES)
def test_resetting_and_quiet_envs_in_one_launch(N, E, env_train):
    """(e) the oracle alone says first which envs reset somebody in which step: steps with both kinds of env in
    the launch - and, at 16 / 32 drones, inside one wave - must occur."""
    T = 4
    world = _mixed_world(E, N)
    ref = orc.OracleEnv(world.waypoints, world.n_points, world.map_size, world.buildings, nm=10, threads=8,
                        env_train=env_train)
    ref.observe()
    mixed_launch = mixed_wave = 0
    epw = 64 // (64 if N == 48 else N)  # envs per wave
    for t in range(T):
        rm = ref.step_autoreset(synthetic_actions(E, N, t, SEED))[6].reshape(E, N).any(axis=1)
        mixed_launch += int(rm.any() and not rm.all())
        waves = rm[:E - E % epw].reshape(-1, epw)
        mixed_wave += int((waves.any(axis=1) & ~waves.all(axis=1)).any())
    assert mixed_launch >= 1 and (epw == 1 or mixed_wave >= 1), (mixed_launch, mixed_wave)
    st = run_vs_oracle(world, T=T, env_train=env_train, seed=SEED, name=f"x1/mixed_{N}x{E}_t{int(env_train)}")
    assert st["resets"] > 0, st
