"""Per-env drone counts (rvo3d_set_drone_counts; BatchedDroneEnv.set_drone_counts, World.drone_counts) on the GPU.

Yardstick: the existing, oracle-pinned path (test_gpu_parity.py).  For every distinct count c of a counted handle a plain
handle with num_drones = c is built over the envs of that count (World.select, drones [:c]); the counted handle's live rows
must equal it bit for bit - np.array_equal with NaN == NaN, no tolerance, no exempt rows - after every call: obs, reward,
vo_count, done, info, finish, reset_mask and all ten state fields.  The library is built with -ffp-contract=off and
decides in float64 behind conservative float32 filters, so which ring a fleet runs on must not show in any bit.  The ghost
rows must hold their defined values (zeros) although every output buffer of the counted handle is filled with 0xFF bytes
before every call (reuse_obs=False), and the ghosts' action rows are NaN.

Scene: crossing_world(E, N, (30, 30, 8), radius = 4 if N <= 16 else 6 if N <= 64 else 11, min_sep = 0.5 if N <= 100 else
0.45, alt_spread = 1.0 if N <= 100 else 2.5, seed = 41), 25 steps, neighbors_num 10, env_train = True, both autoreset
settings; every handle is steered by its own follow() (the rule of tests/test_gpu_routes.py, restated below).  Counts are
cycled over the envs:

    8 x 21    (8, 1, 3, 5, 2, 8, 7)       several envs per wave, partial last workgroup, count 1
    32 x 6    (32, 22, 31, 1, 16, 27)
    64 x 6    (64, 33, 48, 1, 63, 2)      the yardsticks of 33, 48 and 63 run the padded-64 kernel themselves
    100 x 3   (100, 65, 7)                two waves
    256 x 3   (256, 129, 40)              four waves

The comparison is not vacuous: a full handle without counts runs beside the counted one, and the CPU oracle on exactly these
inputs gave (truncated envs; "differ": live rows of envs with c < N whose observation differs from the full env's;
knife-edge: rows with an oracle margin below 1e-9):

    shape, autoreset     rows with VO   done          finish      resets     differ      knife-edge rows
    8 x 21, off / on     10 / 9         189 / 254     1033 / 16   - / 270    5 / 311     0 / 0
    32 x 6               62 / 17        816 / 324     272 / 2     - / 326    15 / 150    0 / 0
    64 x 6               169 / 26       2068 / 688    407 / 2     - / 690    22 / 201    0 / 0
    100 x 3              146 / 26       1935 / 222    0 / 0       - / 222    36 / 46     0 / 0
    256 x 3              468 / 4        5343 / 740    0 / 0       - / 740    150 / 150   0 / 1

The tests assert > 0 for VO rows, done and differ in every line, and for resets with autoreset on.

Worlds with buildings (crossing_world has none): synthetic_world(E, N, map, n_points = 2, nb, seed = 41, min_sep = 0.6), the
buildings one shared list (the xy grid, grid cells that overflow) or a set per env (read through bld_stride /
bgrid_stride) whose sizes set_sizes() draws: env 0 has all nb, env 2 none.  The same yardstick - plain handles, which
test_gpu_parity.py pins to the CPU oracle in worlds with buildings -, 25 steps, both autoreset settings:

    N x E      counts                     map            nb   buildings
    21 x 8     (21, 1, 3, 5, 2, 8, 7)     (12, 12, 5)    3    shared, per-env     L = 32 lanes per env, eight envs a workgroup
    64 x 6     (64, 33, 48, 1, 63, 2)     (16, 16, 6)    4    per-env             a full wave per env
    100 x 3    (100, 65, 7)               (20, 20, 8)    6    shared, per-env     two waves
    256 x 3    (256, 129, 40)             (40, 40, 10)   10   per-env             four waves

What the GPU run tallied (autoreset off / on; "done at a building": live rows whose `done` coincides with bclear <= 0 in
safety_numpy on the handle's own positions - behind plain steps only, an auto-resetting step has moved the drone away):

    scene                rows with VO   done        done at a building   finish       resets     differ
    21 x 8 shared        4 / 2          272 / 319   257 / -              1023 / 99    - / 407    0 / 60
    21 x 8 per-env       4 / 2          210 / 245   193 / -              1023 / 114   - / 350    0 / 115
    64 x 6 per-env       21 / 8         583 / 603   448 / -              2229 / 251   - / 836    4 / 252
    100 x 3 shared       15 / 8         437 / 579   376 / -              1373 / 148   - / 715    1 / 130
    100 x 3 per-env      15 / 7         443 / 461   381 / -              1373 / 155   - / 604    1 / 90
    256 x 3 per-env      15 / 5         484 / 563   404 / -              796 / 112    - / 675    5 / 242

The CPU oracle, every env run alone at its count, gives the same figures.  The tests assert > 0 for VO rows, done and
finish in every run, for done at a building behind plain steps, and for resets and differ with autoreset on: these
drones fly apart from each other, so behind plain steps - where a drone that is `done` stays where it is - a fleet cut
down to c drones sees what the full fleet sees in all but a few rows, and in none at 21 x 8.

Two more tests at 21 x 8 with per-env sets attach the counts and the sets in either order (rvo3d_set_env_buildings and
rvo3d_set_drone_counts each rebuild the device's Cold block and carry the other call's fields over), 10 auto-resetting
steps against the same yardsticks; the second replaces the sets after step 5 (seed 42) on every handle.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, World, _lib
from rvo3d_amd.safety import safety_numpy
from rvo3d_amd.worlds import crossing_world, synthetic_world

pytestmark = pytest.mark.gpu

CASES = {(8, 21): (8, 1, 3, 5, 2, 8, 7), (32, 6): (32, 22, 31, 1, 16, 27), (64, 6): (64, 33, 48, 1, 63, 2),
         (100, 3): (100, 65, 7), (256, 3): (256, 129, 40)}
SMALL = [(8, 21), (64, 6)]
# worlds with buildings (module docstring): (N, E) -> (counts, map, nb); (N, E, per-env sets)
BLD_CASES = {(21, 8): ((21, 1, 3, 5, 2, 8, 7), (12.0, 12.0, 5.0), 3), (64, 6): ((64, 33, 48, 1, 63, 2), (16.0, 16.0, 6.0), 4),
             (100, 3): ((100, 65, 7), (20.0, 20.0, 8.0), 6), (256, 3): ((256, 129, 40), (40.0, 40.0, 10.0), 10)}
BLD_SCENES = [(21, 8, False), (21, 8, True), (64, 6, True), (100, 3, False), (100, 3, True), (256, 3, True)]
OUT_KEYS = ("obs", "vo_count", "reward", "done", "info", "finish", "reset_mask")
STATE_KEYS = ("pos", "vel", "yaw", "pitch", "real_len", "max_dev", "extra_len", "wp_idx", "arrive", "dest")
STEPS = 25
INVALID, STATE = -1, -3


def host(t):
    return t.cpu().numpy()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@functools.lru_cache(maxsize=None)
def scene(N, E):
    return crossing_world(E, N, (30.0, 30.0, 8.0), radius=4 if N <= 16 else 6 if N <= 64 else 11,
                          min_sep=0.5 if N <= 100 else 0.45, alt_spread=1.0 if N <= 100 else 2.5, seed=41)


def cycled(N, E, cyc=None):
    cyc = CASES[(N, E)] if cyc is None else cyc
    return np.array([cyc[e % len(cyc)] for e in range(E)], dtype=np.int32)


def set_sizes(E, nb, seed=41):
    """building_counts of a per-env scene: env 0 has all nb buildings, env 2 none, the others a drawn number."""
    c = np.random.default_rng(seed).integers(0, nb + 1, E).astype(np.int32)
    c[0], c[2] = nb, 0
    return c


@functools.lru_cache(maxsize=None)
def building_scene(N, E, per_env, seed=41):
    """synthetic_world with nb buildings - one shared list, or a set per env with set_sizes - and the cycled counts."""
    cyc, m, nb = BLD_CASES[(N, E)]
    w = synthetic_world(E, N, m, n_points=2, nb=nb, seed=seed, min_sep=0.6, per_env_buildings=per_env)
    if per_env:
        w = World(w.waypoints, w.n_points, w.map_size, w.buildings, set_sizes(E, nb))
    return w, cycled(N, E, cyc)


def truncated(world, envs, c):
    """The world of the listed envs with their first c drones; per-env building sets keep their building_counts."""
    w = world.select(envs)
    return World(w.waypoints[:, :c].copy(), w.n_points[:, :c].copy(), w.map_size, w.buildings, w.building_counts)


def yardsticks(world, counts, **kw):
    """{c: (envs, plain handle of num_drones = c over the envs whose count is c)}"""
    out = {}
    for c in sorted(set(int(x) for x in counts)):
        envs = np.nonzero(counts == c)[0]
        out[c] = (envs, BatchedDroneEnv(truncated(world, envs, c), **kw))
    return out


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


def follow_counted(env):
    """follow() with NaN in the ghosts' action rows."""
    a = follow(env)
    a[~env.live] = float("nan")
    return a


def poison(env, keys=OUT_KEYS):
    """0xFF in every byte of the handle's output buffers: what a call does not write stays visible."""
    for k in keys:
        getattr(env, k).view(torch.uint8).fill_(0xFF)


def outputs(env, keys):
    out = {k: host(getattr(env, k)) for k in keys}
    out.update({k: host(v) for k, v in env.get_state().items()})
    return out


def check_counted(K, Y, counts, keys, what, world=None):
    """The counted handle's live rows against the yardsticks, its ghost rows against their defined values; with `world`
    the ghosts' state against the reset state of their unused routes."""
    got = outputs(K, keys)
    N = K.N
    for c, (envs, y) in Y.items():
        want = outputs(y, keys)
        for k in list(keys) + list(STATE_KEYS):
            assert same(got[k][envs, :c], want[k]), f"{what}: {k} of the envs with {c} drones"
    ghost = np.arange(N)[None, :] >= counts[:, None]
    for k in keys:
        assert not np.any(got[k][ghost].view(np.uint8)), f"{what}: ghost rows of {k}"
    if world is not None:
        assert same(got["pos"][ghost], world.waypoints[:, :, 0][ghost]), f"{what}: ghost positions"
        for k in ("vel", "yaw", "pitch", "real_len", "arrive", "dest"):
            assert not np.any(got[k][ghost]), f"{what}: ghost state {k}"
        assert np.all(got["wp_idx"][ghost] == 1), f"{what}: ghost wp_idx"
    return got


@functools.lru_cache(maxsize=None)
def run(N, E, autoreset, env_train=True):
    """The comparison of the module docstring; returns the tallies the tests assert on."""
    return run_world(scene(N, E), cycled(N, E), autoreset, env_train)


@functools.lru_cache(maxsize=None)
def run_buildings(N, E, per_env, autoreset):
    return run_world(*building_scene(N, E, per_env), autoreset)


def run_world(world, counts, autoreset, env_train=True):
    """run() on any world.  With buildings the tally `bdone` counts the live rows whose `done` coincides with
    bclear <= 0 in safety_numpy on the handle's own positions - behind plain steps only: an auto-resetting step has
    moved every `done` drone to its start before anybody can look."""
    N, E = world.shape[1], world.shape[0]
    has_bld = np.size(world.buildings) > 0
    K = BatchedDroneEnv(world.with_drone_counts(counts), env_train=env_train, reuse_obs=False)
    F = BatchedDroneEnv(world, env_train=env_train)
    Y = yardsticks(world, counts, env_train=env_train)
    assert "env_kernel_counted" in K.kernel_name() and "counted" not in F.kernel_name()
    keys = OUT_KEYS if autoreset else OUT_KEYS[:-1]   # (the plain step hands out a reset mask only with auto-reset)
    poison(K)
    for x in [K, F] + [y for _, y in Y.values()]:
        x.observe()
    check_counted(K, Y, counts, ("obs", "vo_count"), "observe", world)
    tally = dict(vo=0, done=0, bdone=0, finish=0, resets=0, differ=0)
    part = np.arange(N)[None, :] < np.where(counts < N, counts, 0)[:, None]   # live rows of the envs with c < N
    for t in range(STEPS):
        acts = [(K, follow_counted(K)), (F, follow(F))] + [(y, follow(y)) for _, y in Y.values()]
        poison(K)
        for x, a in acts:
            x.step(a, autoreset=autoreset)
        got = check_counted(K, Y, counts, keys, f"step {t}", world)
        live = np.arange(N)[None, :] < counts[:, None]
        tally["vo"] += int(np.sum(got["vo_count"][live] > 0))
        tally["done"] += int(np.sum(got["done"][live] != 0))
        tally["finish"] += int(np.sum(got["finish"][live] != 0))
        if autoreset:
            tally["resets"] += int(np.sum(got["reset_mask"][live] != 0))
        elif has_bld:
            bclear = safety_numpy(got["pos"], 0.2, world.map_size, 0.5, counts=counts, buildings=world.buildings,
                                  building_counts=world.building_counts)[1]
            tally["bdone"] += int(np.sum((got["done"][live] != 0) & (bclear[live] <= 0)))
        tally["differ"] += int(np.sum(np.any(got["obs"] != host(F.obs), axis=-1) & part))
    # the error word: what the yardsticks raised between them (env_train off: the reference's math domain error)
    want = 0
    for _, y in Y.values():
        want |= y.error_flags()
    assert K.error_flags() == want and (want == 0 or not env_train)
    for x in [K, F] + [y for _, y in Y.values()]:
        x.close()
    return tally


@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("N,E", list(CASES))
def test_counted_envs_equal_plain_handles_of_their_size(N, E, autoreset):
    tally = run(N, E, autoreset)
    print(f"{N} x {E}, autoreset {autoreset}: {tally}")
    assert tally["vo"] > 0 and tally["done"] > 0 and tally["differ"] > 0, tally
    if autoreset:
        assert tally["resets"] > 0, tally


@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("N,E,per_env", BLD_SCENES)
def test_counted_envs_in_worlds_with_buildings(N, E, per_env, autoreset):
    """env_kernel_counted along the building path: the shared list with its xy grid, and per-env sets read through
    bld_stride / bgrid_stride, one of them empty and one full."""
    world, counts = building_scene(N, E, per_env)
    if per_env:
        assert world.per_env_buildings and 0 in world.building_counts and world.buildings.shape[1] in world.building_counts
    tally = run_buildings(N, E, per_env, autoreset)
    print(f"{N} x {E}, {'per-env sets' if per_env else 'shared list'}, autoreset {autoreset}: {tally}")
    assert tally["vo"] > 0 and tally["done"] > 0 and tally["finish"] > 0, tally
    if autoreset:
        assert tally["resets"] > 0 and tally["differ"] > 0, tally
    else:   # (plain steps: the drones of these scenes stay apart, 21 x 8 has no row that differs - module docstring)
        assert tally["bdone"] > 0, tally


def other_sets(E, N, seed=42):
    """Per-env sets for the 21 x 8 scene from another seed, with the scene's set sizes."""
    _, m, nb = BLD_CASES[(N, E)]
    return synthetic_world(E, 1, m, nb=nb, seed=seed, per_env_buildings=True).buildings


def ordering_run(K, world, counts, swap_at=None):
    """10 auto-resetting steps of the counted handle K against the yardsticks of `world`, beside K0, a counted handle
    that never had a building (and, from swap_at on, beside K1, a counted handle that keeps the first sets while K and
    the yardsticks get other_sets).  Returns the rows whose `done` differs from K0's, and at step swap_at from K1's."""
    N, E = world.shape[1], world.shape[0]
    Y = yardsticks(world, counts)
    K0 = BatchedDroneEnv(World(world.waypoints, world.n_points, world.map_size).with_drone_counts(counts))
    K1 = BatchedDroneEnv(world.with_drone_counts(counts)) if swap_at is not None else None
    assert "env_kernel_counted" in K.kernel_name()
    handles = [K, K0] + ([K1] if K1 else []) + [y for _, y in Y.values()]
    poison(K)
    for x in handles:
        x.observe()
    check_counted(K, Y, counts, ("obs", "vo_count"), "observe", world)
    live = np.arange(N)[None, :] < counts[:, None]
    built = swapped = 0
    for t in range(10):
        if t == swap_at:
            new = other_sets(E, N)
            K.set_env_buildings(new, world.building_counts)
            for envs, y in Y.values():
                y.set_env_buildings(new[envs], world.building_counts[envs])
        acts = [(x, follow_counted(x) if x.drone_counts is not None else follow(x)) for x in handles]
        poison(K)
        for x, a in acts:
            x.step(a, autoreset=True)
        got = check_counted(K, Y, counts, OUT_KEYS, f"step {t}", world)
        built += int(np.sum((got["done"] != host(K0.done))[live]))
        if t == swap_at:
            swapped = int(np.sum((got["done"] != host(K1.done))[live]))
    assert K.error_flags() == 0
    for x in handles:
        x.close()
    return built, swapped


def test_counts_first_then_env_buildings():
    """rvo3d_set_env_buildings on a counted handle: the Cold block it rebuilds keeps the counts."""
    world, counts = building_scene(21, 8, True)
    K = BatchedDroneEnv(World(world.waypoints, world.n_points, world.map_size).with_drone_counts(counts), reuse_obs=False)
    K.set_env_buildings(world.buildings, world.building_counts)
    built, _ = ordering_run(K, world, counts)
    print(f"counts first: rows whose done differs from a handle without buildings {built}")
    assert built > 0


def test_env_buildings_first_then_counts():
    """rvo3d_set_drone_counts on a handle of per-env sets: the Cold block it rebuilds keeps the sets; new sets after
    step 5 show in the very next step."""
    world, counts = building_scene(21, 8, True)
    K = BatchedDroneEnv(world, reuse_obs=False)
    K.set_drone_counts(counts)
    built, swapped = ordering_run(K, world, counts, swap_at=5)
    print(f"buildings first: rows whose done differs from a handle without buildings {built}, "
          f"from a handle that kept the old sets at the step behind the swap {swapped}")
    assert built > 0 and swapped > 0


@pytest.mark.parametrize("autoreset", [False, True])
def test_counted_envs_with_env_train_off(autoreset):
    tally = run(64, 6, autoreset, env_train=False)
    print(f"64 x 6, env_train off, autoreset {autoreset}: {tally}")
    assert tally["done"] > 0 and tally["differ"] > 0, tally


@pytest.mark.parametrize("N,E", SMALL)
def test_step_policy_with_reused_observation_buffers(N, E):
    """step_policy (float32 increments) with reuse_obs=True - the prev_vo_count promise - equals reuse_obs=False bit
    for bit over 25 steps; the ghosts' increments are NaN.  The increments are follow()'s steering put through the
    inverse of the trainer's glue, (action - vel) / acceler as float32: random increments bring no drones together, and
    it is the rows with velocity obstacles that the promise is about."""
    world, counts = scene(N, E).with_drone_counts(cycled(N, E)), cycled(N, E)
    A, B = BatchedDroneEnv(world, reuse_obs=True), BatchedDroneEnv(world, reuse_obs=False)
    for x in (A, B):
        x.observe()
    vo = 0
    for t in range(STEPS):
        a = ((follow(A) - A.vel) / A.acceler).float()
        a[~A.live] = float("nan")
        poison(B)
        for x in (A, B):
            x.step_policy(a, autoreset=True)
        for k in OUT_KEYS:
            assert same(host(getattr(A, k)), host(getattr(B, k))), (t, k)
        sa, sb = A.get_state(), B.get_state()
        for k in STATE_KEYS:
            assert same(host(sa[k]), host(sb[k])), (t, k)
        vo += int((A.vo_count > 0).sum())
    print(f"{N} x {E}: rows with VO {vo}")
    assert vo > 0
    ghost = np.arange(N)[None, :] >= counts[:, None]
    assert not np.any(host(A.obs)[ghost]) and not np.any(host(A.vo_count)[ghost])
    A.close(); B.close()


@pytest.mark.parametrize("N,E", SMALL)
def test_set_drone_counts_in_mid_run(N, E):
    """At step 7 some counts go up and some down: the changed envs equal fresh handles of the new size, the others go on
    bit for bit as in a handle that never got the call; None brings the full envs back."""
    world, c1 = scene(N, E), cycled(N, E)
    c2 = c1.copy()
    c2[0::3] = np.roll(c1, 1)[0::3]            # every third env takes its neighbour's count: ups and downs
    changed = c1 != c2
    assert changed.any() and (~changed).any() and (c2[changed] > c1[changed]).any() and (c2[changed] < c1[changed]).any()
    K, K0 = BatchedDroneEnv(world.with_drone_counts(c1)), BatchedDroneEnv(world.with_drone_counts(c1))
    for x in (K, K0):
        x.observe()
    for t in range(7):
        for x in (K, K0):
            x.step(follow_counted(x), autoreset=True)
    K.set_drone_counts(c2)
    assert same(host(K.drone_counts), c2) and same(host(K.live), np.arange(N)[None, :] < c2[:, None])
    Y = yardsticks(world.select(np.nonzero(changed)[0]), c2[changed])
    for x in [K, K0] + [y for _, y in Y.values()]:
        x.observe()
    same_envs, ch = np.nonzero(~changed)[0], np.nonzero(changed)[0]

    def check(what):
        got, want0 = outputs(K, OUT_KEYS), outputs(K0, OUT_KEYS)
        for k in got:
            assert same(got[k][same_envs], want0[k][same_envs]), f"{what}: {k} of the unchanged envs"
        for c, (envs, y) in Y.items():
            want = outputs(y, OUT_KEYS)
            for k in got:
                assert same(got[k][ch[envs], :c], want[k]), f"{what}: {k} of the envs that now have {c} drones"
        ghost = np.arange(N)[None, :] >= c2[:, None]
        for k in OUT_KEYS:
            assert not np.any(got[k][ghost]), f"{what}: ghost rows of {k}"

    for t in range(7, 15):
        for x in [K, K0] + [y for _, y in Y.values()]:
            x.step(follow_counted(x) if x in (K, K0) else follow(x), autoreset=True)
        check(f"step {t}")
    # None: every env whose count was below N is a full env in its reset state again
    K.set_drone_counts(None)
    assert K.drone_counts is None and bool(K.live.all()) and "counted" not in K.kernel_name()
    F = BatchedDroneEnv(world)
    part = np.nonzero(c2 < N)[0]
    for x in (K, F):
        x.observe()
    for t in range(5):
        for x in (K, F):
            x.step(follow(x), autoreset=True)
        got, want = outputs(K, OUT_KEYS), outputs(F, OUT_KEYS)
        for k in got:
            assert same(got[k][part], want[k][part]), f"after None, step {t}: {k}"
    for x in [K, K0, F] + [y for _, y in Y.values()]:
        x.close()


@pytest.mark.parametrize("N,E", SMALL)
def test_entry_points_of_a_counted_handle(N, E):
    """reset_drones with ghost bytes set, reset(env_mask), observe_envs, des_vel, rvo_vel and set_routes against the
    yardsticks."""
    world, counts = scene(N, E), cycled(N, E)
    K = BatchedDroneEnv(world.with_drone_counts(counts), reuse_obs=False)
    Y = yardsticks(world, counts)
    handles = [K] + [y for _, y in Y.values()]
    ghost = np.arange(N)[None, :] >= counts[:, None]
    for x in handles:
        x.observe()
    for t in range(6):
        for x in handles:
            x.step(follow_counted(x) if x is K else follow(x), autoreset=False)
    check_counted(K, Y, counts, OUT_KEYS[:-1], "before the calls", world)

    def vectors(fn, what):
        got = host(fn(K))
        for c, (envs, y) in Y.items():
            assert same(got[envs, :c], host(fn(y))), f"{what} of the envs with {c} drones"
        assert not np.any(got[ghost].view(np.uint8)), f"{what}: ghost rows"

    vectors(lambda x: x.des_vel(), "des_vel")
    vectors(lambda x: x.rvo_vel(), "rvo_vel")
    rng = np.random.default_rng(3)
    # reset_drones: every ghost byte set, a third of the live ones
    m = rng.uniform(size=(E, N)) < 0.33
    K.reset_drones(torch.from_numpy(m | ghost).cuda())
    for c, (envs, y) in Y.items():
        y.reset_drones(torch.from_numpy(m[envs, :c]).cuda())
    poison(K, ("obs", "vo_count"))
    for x in handles:
        x.observe()
    check_counted(K, Y, counts, ("obs", "vo_count"), "reset_drones", world)
    for x in handles:
        x.step(follow_counted(x) if x is K else follow(x), autoreset=True)
    # reset(env_mask) + observe_envs
    em = np.arange(E) % 2 == 0
    K.reset(torch.from_numpy(em).cuda())
    K.observe_envs(torch.from_numpy(em).cuda())
    for c, (envs, y) in Y.items():
        y.reset(torch.from_numpy(em[envs]).cuda())
        y.observe_envs(torch.from_numpy(em[envs]).cuda())
    check_counted(K, Y, counts, ("obs", "vo_count"), "reset + observe_envs", world)
    # set_routes: the routes reversed; a bad n_points in a ghost row raises nothing ...
    wp = np.ascontiguousarray(world.waypoints[:, :, ::-1])
    npts = np.array(world.n_points)
    bad = npts.copy()
    bad[ghost] = 99
    assert ghost.any()
    K.set_routes(wp, bad)
    assert K.error_flags() == 0
    for c, (envs, y) in Y.items():
        y.set_routes(wp[envs, :c], npts[envs, :c])
    poison(K, ("obs", "vo_count"))
    for x in handles:
        x.observe()
    got = check_counted(K, Y, counts, ("obs", "vo_count"), "set_routes")
    assert same(got["pos"][ghost], world.waypoints[:, :, 0][ghost]), "the ghosts kept their routes"
    # ... and in a live row the flag, and its env keeps what it had
    bad = npts.copy()
    bad[1, 0] = 1
    K.set_routes(np.ascontiguousarray(world.waypoints), bad)
    assert K.error_flags() == 4
    for c, (envs, y) in Y.items():
        keep = envs != 1
        if keep.any():
            y.set_routes(world.waypoints[envs, :c], npts[envs, :c], keep)
    for x in handles:
        x.observe()
    check_counted(K, Y, counts, ("obs", "vo_count"), "set_routes with a bad live row")
    for x in handles:
        x.close()


def eval_loop(env, steps, max_ep_len, quota):
    """The fused evaluator's loop (post_train) driven by des_vel: returns the records and the running values."""
    E, dev = env.E, env.device
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    t = dict(ep_len=z(E, torch.int32), ep_ret=z(E, torch.float64), speed_sum=z(E, torch.float64),
             counted=z(E, torch.int32), rec_len=z((E, quota), torch.int32), rec_ret=z((E, quota), torch.float64),
             rec_speed=z((E, quota), torch.float64), rec_step=z((E, quota), torch.int64),
             rec_flags=z((E, quota), torch.uint8), remaining=torch.full((1,), quota * E, dtype=torch.int32, device=dev),
             ended=z(E, torch.uint8))
    bufs = _lib.EvalBufs(**{k: v.data_ptr() for k, v in t.items()})
    p = lambda x: C.c_void_p(x.data_ptr())
    env.reset()
    env.observe()
    for step in range(steps):
        a32 = follow(env).float()
        a32[~env.live] = float("nan")
        act = env.eval_action(a32, 1.0)
        if step == 3:
            act3 = host(act)
        _, _, rew, done, info, fin = env.step(follow_counted(env))
        _lib.check(_lib.lib().rvo3d_eval_account(env._h, p(rew), p(done), p(info), p(fin), max_ep_len, quota, step,
                                                 C.byref(bufs), env._stream()), "rvo3d_eval_account")
        env.reset(t["ended"])
        env.observe_envs(t["ended"])
    out = {k: host(v) for k, v in t.items() if k != "remaining"}
    out["eval_action"] = act3
    return out


@pytest.mark.parametrize("N,E", SMALL)
def test_eval_account_records_equal_the_yardsticks(N, E):
    world, counts = scene(N, E), cycled(N, E)
    K = BatchedDroneEnv(world.with_drone_counts(counts))
    got = eval_loop(K, STEPS, 10, 2)
    assert got["counted"].sum() > 0
    act = got.pop("eval_action")
    assert not np.any(act[np.arange(N)[None, :] >= counts[:, None]].view(np.uint8)), "eval_action: ghost rows"
    for c, (envs, y) in yardsticks(world, counts).items():
        want = eval_loop(y, STEPS, 10, 2)
        assert same(act[envs, :c], want.pop("eval_action")), f"eval_action of the envs with {c} drones"
        for k in got:
            assert same(got[k][envs], want[k]), f"{k} of the envs with {c} drones"
        y.close()
    K.close()


def account_numpy(st, counts, rew, done, fin, max_ep_len, epoch_end):
    """rvo3d_rollout_account_n restated (multi_ppo.py:217-281 over the live drones); st: ep_ret, ep_len, sums."""
    E, N = rew.shape
    live = np.arange(N)[None, :] < counts[:, None]
    rf = np.where(np.isfinite(rew), rew, np.float32(0)).astype(np.float32)
    ret = (st["ep_ret"] + rf).astype(np.float32)
    length = st["ep_len"] + 1
    by_step = (fin != 0) | (done != 0)
    timeout = length > max_ep_len
    ended = (by_step | timeout | bool(epoch_end)) & live
    extra = (timeout | bool(epoch_end)) & ~by_step & live
    cut = (((fin != 0) | timeout) & live).any(axis=1) | bool(epoch_end)
    st["sums"][:, 0] += np.where(ended, ret.astype(np.float64), 0.0).sum(axis=1)
    st["sums"][:, 1] += ended.sum(axis=1)
    st["ep_ret"] = np.where(live, np.where(ended, np.float32(0), ret), st["ep_ret"]).astype(np.float32)
    st["ep_len"] = np.where(live, np.where(ended, 0, length), st["ep_len"]).astype(np.int32)
    return np.where(live, rf, np.float32(0)), cut.astype(np.uint8), extra.astype(np.uint8)


def test_rollout_account_n_against_numpy():
    """max_ep_len 5 over 12 calls: the ghosts never cut, never enter sums and never set any_extra; with NULL counts the
    call equals rvo3d_rollout_account bit for bit."""
    N, E = 8, 21
    counts = cycled(N, E)
    live = np.arange(N)[None, :] < counts[:, None]
    rng = np.random.default_rng(9)
    L = _lib.lib()
    p = lambda x: C.c_void_p(x.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def fresh():
        return dict(rew_slot=torch.full((E, N), 7.0, device="cuda"), ep_ret=torch.zeros((E, N), device="cuda"),
                    ep_len=torch.zeros((E, N), dtype=torch.int32, device="cuda"),
                    cut=torch.zeros(E, dtype=torch.uint8, device="cuda"),
                    extra=torch.full((E, N), 9, dtype=torch.uint8, device="cuda"),
                    sums=torch.zeros((E, 2), dtype=torch.float64, device="cuda"),
                    any_extra=torch.zeros(1, dtype=torch.int32, device="cuda"))

    def call(b, cnt, rew, done, fin, epoch_end, n=True):
        args = [p(rew), p(done), p(fin), 1, 5, epoch_end, p(b["rew_slot"]), p(b["ep_ret"]), p(b["ep_len"]), p(b["cut"]),
                p(b["extra"]), p(b["sums"]), p(b["any_extra"]), None]
        if n:
            _lib.check(L.rvo3d_rollout_account_n(E, N, None if cnt is None else p(cnt), *args), "rvo3d_rollout_account_n")
        else:
            _lib.check(L.rvo3d_rollout_account(E, N, *args), "rvo3d_rollout_account")

    cdev = dev(counts)
    b, b_null, b_old = fresh(), fresh(), fresh()
    st = dict(ep_ret=np.zeros((E, N), np.float32), ep_len=np.zeros((E, N), np.int32), sums=np.zeros((E, 2)))
    timeouts, sticky = 0, False
    for t in range(12):
        rew = rng.normal(0, 3, (E, N)).astype(np.float32)
        rew[rng.uniform(size=(E, N)) < 0.05] = np.nan
        done = (rng.uniform(size=(E, N)) < 0.03).astype(np.uint8)
        fin = (rng.uniform(size=(E, N)) < 0.02).astype(np.uint8)
        # the step's outputs of a ghost are zeros; here they are set, so that a kernel that looked at them would show
        rew_g, done_g, fin_g = rew.copy(), done.copy(), fin.copy()
        done[~live] = 0; fin[~live] = 0
        done_g[~live] = 1; fin_g[~live] = 1; rew_g[~live] = 100.0
        epoch_end = 1 if t == 11 else 0
        for x in (b, b_null, b_old):
            x["cut"].zero_()
        call(b, cdev, dev(rew_g), dev(done_g), dev(fin_g), epoch_end)
        call(b_null, None, dev(rew), dev(done), dev(fin), epoch_end)
        call(b_old, None, dev(rew), dev(done), dev(fin), epoch_end, n=False)
        timeouts += int(((st["ep_len"] + 1 > 5) & live).sum())
        slot, cut, extra = account_numpy(st, counts, rew, done, fin, 5, epoch_end)
        assert same(host(b["rew_slot"]), slot) and same(host(b["cut"]), cut) and same(host(b["extra"]), extra), t
        assert same(host(b["ep_ret"]), st["ep_ret"]) and same(host(b["ep_len"]), st["ep_len"]), t
        np.testing.assert_allclose(host(b["sums"]), st["sums"], rtol=1e-12)
        sticky = sticky or bool(extra.any())
        assert int(b["any_extra"].item()) == int(sticky), t
        for k in b_null:
            assert same(host(b_null[k]), host(b_old[k])), (t, k)
    assert timeouts > 0
    assert not np.any(host(b["ep_len"])[~live]) and not np.any(host(b["ep_ret"])[~live])
    # ghosts alone never raise any_extra: every live drone is reset by the step, every ghost byte says "timed out"
    b2 = fresh()
    b2["ep_len"].fill_(100)
    b2["ep_len"][torch.from_numpy(live).cuda()] = 0
    one = np.ones((E, N), np.uint8)
    call(b2, cdev, dev(np.zeros((E, N), np.float32)), dev(one), dev(one), 0)
    assert int(b2["any_extra"].item()) == 0 and not np.any(host(b2["extra"]))
    assert np.all(host(b2["sums"])[:, 1] == counts)


@pytest.mark.parametrize("fused", [True, False])
def test_one_trainer_epoch_on_a_counted_env(fused):
    from rvo3d_amd.policy import mlp_ac, multi_ppo
    N, E, T = 8, 21, 8
    counts = cycled(N, E)
    env = BatchedDroneEnv(scene(N, E).with_drone_counts(counts))
    env.observe()
    torch.manual_seed(3)
    ac = mlp_ac(env.W).cuda()
    tr = multi_ppo(env, ac, steps_per_epoch=T, max_ep_len=5, train_pi_iters=2, train_v_iters=2, seed=3, tune_gemms=False,
                   fused_rollout=fused)
    assert tr.robot_num == int(counts.max())
    mean_ret = tr.collect()
    live = host(env.live)
    assert not np.any(host(tr.ep_len)[~live]) and not np.any(host(tr.buf.rew)[:, ~live])
    data = tr.buf.get()
    rows = T * int(counts.sum())
    assert data["shape"] == (T, E, N) and same(host(data["live"]), live)
    for k in ("obs", "cnt", "act", "ret", "adv", "logp"):
        assert data[k].shape[0] == rows, k
    assert same(host(data["obs"]), host(tr.buf.obs[:T])[:, live].reshape(rows, -1))
    assert np.isfinite(mean_ret)
    stats = tr.update(data)
    assert np.isfinite(stats["loss_v"])
    env.close()


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_statistic_is_the_live_drones_episodes(fused):
    """The logged episodes, their summed return and the path cuts of one epoch, fused and module rollout, against the
    trainer's rules (multi_ppo.py:217-281) restated over the live drones from what the steps returned: max_ep_len 5 in
    8 steps, so drones time out, and the epoch ends every path.  A ghost that timed out, ended a path or counted as an
    episode would show in each of the three."""
    from rvo3d_amd.policy import mlp_ac, multi_ppo
    N, E, T, max_ep_len = 8, 21, 8, 5
    counts = cycled(N, E)
    env = BatchedDroneEnv(scene(N, E).with_drone_counts(counts))
    env.observe()
    torch.manual_seed(3)
    tr = multi_ppo(env, mlp_ac(env.W).cuda(), steps_per_epoch=T, max_ep_len=max_ep_len, seed=3, tune_gemms=False,
                   fused_rollout=fused)
    flags = []
    step_policy = env.step_policy

    def recording(*a, **kw):
        out = step_policy(*a, **kw)
        flags.append((host(env.done) != 0, host(env.finish) != 0))
        return out

    env.step_policy = recording
    mean_ret = tr.collect()
    live = host(env.live)
    rew, cut = host(tr.buf.rew), host(tr.buf.cut)
    ret, length = np.zeros((E, N), np.float32), np.zeros((E, N), np.int64)
    episodes, ret_sum, timeouts = 0, 0.0, 0
    for t, (done, fin) in enumerate(flags):
        ret = (ret + rew[t]).astype(np.float32)
        length += live
        timeout = length > max_ep_len
        ended = (done | fin | timeout | (t == T - 1)) & live
        episodes += int(ended.sum())
        timeouts += int(timeout.sum())
        ret_sum += float(ret[ended].astype(np.float64).sum())
        assert same(cut[t], ((fin | timeout) & live).any(axis=1) | (t == T - 1)), t
        ret[ended] = 0
        length[ended] = 0
    assert len(flags) == T and timeouts > 0
    assert tr.last_rollout["episodes"] == episodes
    np.testing.assert_allclose(tr.last_rollout["ret_sum"], ret_sum, rtol=1e-5)
    np.testing.assert_allclose(mean_ret, ret_sum / episodes, rtol=1e-5)
    assert not np.any(host(tr.ep_len)[~live]) and not np.any(host(tr.ep_ret)[~live])
    env.close()


def test_graph_replayed_rollouts_follow_a_change_of_the_counts():
    """graph_rollout=True with a curriculum: counts -> other counts -> none, two rollouts each (the second of a phase
    replays graphs).  A captured step holds the step kernel, the counts' address and whether the bookkeeping got counts:
    after set_drone_counts + set_live() none of the old graphs may run.  Every rollout must be a faithful one - a second
    env with the same counts, stepped with the stored actions, reproduces every stored observation and reward - and the
    ghosts of the counts in force take no part in the bookkeeping."""
    from rvo3d_amd.policy import mlp_ac, multi_ppo
    N, E, T = 8, 21, 6
    c1 = cycled(N, E)
    c2 = np.roll(c1, 3)
    world = scene(N, E).with_drone_counts(c1)
    env, env2 = BatchedDroneEnv(world), BatchedDroneEnv(world)
    torch.manual_seed(1)
    tr = multi_ppo(env, mlp_ac(env.W).cuda(), steps_per_epoch=T, max_ep_len=50, amp=True, seed=3, graph_rollout=True)
    env.observe()
    o, c = env2.observe()
    nn = lambda x: torch.nan_to_num(x, nan=-7.0)
    for phase, counts in enumerate((c1, c2, None)):
        if phase:
            env.set_drone_counts(counts)
            with pytest.raises(RuntimeError):
                tr.collect(final_reset=False)          # the trainer has not been told
            tr.set_live()
            assert not getattr(tr, "_graphs", None)
            env2.set_drone_counts(counts)
            o, c = env2.observe()
        ghost = torch.zeros((E, N), dtype=torch.bool, device="cuda") if counts is None else ~env.live
        for rollout in range(2):
            tr.buf.ptr = 0
            tr.collect(final_reset=False)
            if not getattr(tr, "_graph_failed", False):
                assert (len(getattr(tr, "_graphs", {})) > 0) == (phase > 0 or rollout >= 1)
            buf = tr.buf
            assert torch.equal(nn(o), nn(buf.obs[0])) and torch.equal(c, buf.cnt[0]), (phase, rollout)
            for t in range(T):
                o, c, rew, done, info, fin = env2.step_policy(buf.act[t], autoreset=True)
                assert torch.equal(nn(o), nn(buf.obs[t + 1])) and torch.equal(c, buf.cnt[t + 1]), (phase, rollout, t)
                assert torch.equal(buf.rew[t], torch.nan_to_num(rew, nan=0.0, posinf=0.0, neginf=0.0)), (phase, rollout, t)
            # the bookkeeping ran on the counts in force: live drones have run since their last reset, ghosts never
            assert not bool(tr.ep_len[ghost].any()) and bool((tr.ep_len[~ghost] > 0).any()), (phase, rollout)
            assert not bool(buf.obs[:, ghost].any()) and not bool(buf.rew[:, ghost].any())
    assert _lib.lib().rvo3d_rollout_set_step_counter(None) == 0
    graphs_refused = getattr(tr, "_graph_failed", False)
    env.close(); env2.close()
    if graphs_refused:
        pytest.skip("this runtime refused the graph capture: the rollouts ran (and were checked) with stream launches")


class _Scripted:
    """A policy that does not look at its observation (the two evaluator loops observe the envs that did not end
    differently, see tests/test_gpu_eval_loop.py): an action per row and call, NaN in the ghosts' rows."""

    def __init__(self, live):
        self.ghost, self.calls = ~live.reshape(-1), 0

    def eval(self):
        return self

    def step_tensors(self, obs, std_factor=1):
        rows = obs[0].shape[0]
        i = torch.arange(rows * 3, device=obs[0].device, dtype=torch.float32).view(rows, 3)
        a = torch.sin(0.37 * i + 1.3 * self.calls) * torch.tensor([1.0, 0.3, 0.15], device=i.device)
        a[self.ghost] = float("nan")
        self.calls += 1
        return a, None, None


def test_post_train_fused_and_host_loop_agree_on_a_counted_env():
    from rvo3d_amd.policy import post_train
    N, E = 8, 21
    got, recs = {}, {}
    for fused in (False, True):
        env = BatchedDroneEnv(scene(N, E).with_drone_counts(cycled(N, E)), env_train=True)
        pt = post_train(env, num_episodes=2 * E, max_ep_len=12, acceler_vel=1.0, inf_print=False, fused=fused)
        got[fused] = pt.policy_test(policy=_Scripted(env.live))
        env.close()
    assert got[True]["episodes"] == got[False]["episodes"] == 2 * E
    assert got[True]["success_rate"] == got[False]["success_rate"]
    assert sorted(got[True]["ep_len"]) == sorted(got[False]["ep_len"])
    np.testing.assert_allclose(sorted(got[True]["speed"]), sorted(got[False]["speed"]), rtol=1e-12)
    np.testing.assert_allclose(sorted(got[True]["ep_ret"]), sorted(got[False]["ep_ret"]), rtol=1e-12)


def test_checkpoint_restores_the_ghosts_routes_too():
    """load_state_dict puts the routes back on full envs before it attaches the counts: a count raised later flies the
    checkpoint's route, not the one the env was built with."""
    N, E = 8, 5
    world = scene(8, 21).select(np.arange(E))
    counts = np.array([3, 8, 1, 5, 2], np.int32)
    env = BatchedDroneEnv(world)
    env.set_routes(np.ascontiguousarray(world.waypoints[:, ::-1]), world.n_points)   # every drone flies another's route
    env.set_drone_counts(counts)
    env.observe()
    for t in range(3):
        env.step(follow_counted(env), autoreset=True)
    sd = env.state_dict()
    env2 = BatchedDroneEnv(world.with_drone_counts(np.full(E, 2, np.int32)))
    env2.load_state_dict(sd)
    assert same(host(env2.drone_counts), counts)
    for a, b in zip(env.routes(), env2.routes()):
        assert same(host(a), host(b))
    for x in (env, env2):
        x.set_drone_counts(None)                 # every ghost becomes a drone: on the checkpoint's routes in both
        x.observe()
    for t in range(3):
        for x in (env, env2):
            x.step(follow(x), autoreset=True)
    part = counts < N
    for k in ("obs", "reward", "done"):
        assert same(host(getattr(env, k))[part], host(getattr(env2, k))[part]), k
    env.close(); env2.close()


def test_argument_edges():
    N, E = 8, 5
    world = scene(8, 21).select(np.arange(E))
    L = _lib.lib()
    hp = lambda a: C.c_void_p(a.ctypes.data)
    env = BatchedDroneEnv(world)
    env.observe()
    before = outputs(env, ("obs", "vo_count"))
    name = env.kernel_name()
    ok = np.full(E, 3, np.int32)
    for bad in (0, N + 1, -1):
        c = ok.copy()
        c[2] = bad
        assert L.rvo3d_set_drone_counts(env._h, hp(c), None) == INVALID
        assert b"counts" in L.rvo3d_last_error()
    assert L.rvo3d_set_drone_counts(None, hp(ok), None) == INVALID
    assert L.rvo3d_set_drone_counts(env._h, None, None) == 0            # NULL on a handle without counts
    ptr = C.c_void_p(1)
    assert L.rvo3d_drone_counts(env._h, C.byref(ptr)) == 0 and not ptr.value
    assert env.kernel_name() == name
    env.observe()
    after = outputs(env, ("obs", "vo_count"))
    for k in before:
        assert same(before[k], after[k]), k                                # the handle is as it was
    with pytest.raises(_lib.RVO3DError):
        env.set_drone_counts(np.zeros(E, np.int32))
    assert env.drone_counts is None
    env.set_drone_counts(ok)
    assert L.rvo3d_drone_counts(env._h, C.byref(ptr)) == 0 and ptr.value
    c = ok.copy()
    c[0] = 0
    assert L.rvo3d_set_drone_counts(env._h, hp(c), None) == INVALID        # refused: the counts in force stay
    assert same(host(env.drone_counts), ok) and "counted" in env.kernel_name()
    sd = env.state_dict()
    assert same(sd["drone_counts"].numpy(), ok)
    env2 = BatchedDroneEnv(world)
    env2.load_state_dict(sd)
    assert same(host(env2.drone_counts), ok)
    env.close(); env2.close()
    # before load_world
    cfg = _lib.Config(E, N, 2, 0, 10, 1, 0, -1, (C.c_double * 3)(30.0, 30.0, 8.0))
    h = C.c_void_p()
    assert L.rvo3d_create(C.byref(cfg), C.byref(h)) == 0
    assert L.rvo3d_set_drone_counts(h, hp(ok), None) == STATE
    L.rvo3d_destroy(h)
    # more drones than the compile-time rings hold
    big = crossing_world(1, 300, (60.0, 60.0, 10.0), radius=25, min_sep=0.3, alt_spread=3.0, seed=41)
    env = BatchedDroneEnv(big)
    assert L.rvo3d_set_drone_counts(env._h, hp(np.full(1, 5, np.int32)), None) == INVALID
    assert b"256" in L.rvo3d_last_error()
    assert "counted" not in env.kernel_name()
    env.close()
