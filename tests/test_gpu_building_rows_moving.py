"""Building rows for moving buildings on the device (include/rvo3d.h: rvo3d_building_rows_moving) against the plain-Python
restatement (tests/building_rows_moving_ref.py on top of building_rows_ref.py and building_motion_ref.py), bit for bit,
and against rvo3d_building_rows on the same state.

The scene (moved_scene; no GPU needed to build it): MAP and NM = 3 of test_gpu_building_rows.py, drones drawn as its scene()
draws them, per-env sets of nb_max = 20 buildings inside the map with counts nb_max - 3, counts[0] = nb_max and
counts[E - 1] = 0, patrols as synthetic_patrols draws them (span 6, speeds 0.3 .. 1.5) with every fourth speed 0 and a NaN
speed for record 5, and three rvo3d_move_env_buildings calls before the rows are taken (dt = 1).  Planted in env 0: drone 0
stands still 1 m ahead of record 1, which comes at it at 1 m per step (urg 0, urg_rel > 0); drone 1 flies 1 m behind record 2
at record 2's own velocity (urg > 0, urg_rel 0) - both close enough to be among the eight nearest of a set of 200.

Shapes (E, N) and what they are there for: (5, 8) the packed geometry; (9, 5) padding lanes inside every env's lane group;
(70, 4) a second, partly filled workgroup; (3, 64) a full wave per env; (2, 130) one workgroup per env, three waves; and
(2, 65) with sets of 200: two record tiles of 128.

Non-vacuity, counted on the CPU from the restatement before any GPU run (tests/test_building_rows_moving_host.py recounts
them without a GPU), among the kept rows at k = 3 / k = 1 - kept rows, rows of a moving building, of one on the arrival
branch (d <= step), rows whose r2(urg_rel) differs from the static r2(urg), rows going from 0 to > 0: TALLY_K3 / TALLY_K1
below."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, BuildingMotion, World, _lib, synthetic_patrols
import building_motion_ref as mref
from building_rows_moving_ref import building_rows_moving_ref

pytestmark = pytest.mark.gpu
MAP = (20.0, 16.0, 8.0)
NM = 3   # W = 39: odd, so are the wide rows of 8k floats - rows that are only 4-byte aligned
DT = 1.0
NB = 20
MOVES = 3
SHAPES = [(5, 8, NB), (9, 5, NB), (70, 4, NB), (3, 64, NB), (2, 130, NB), (2, 65, 200)]
# (E, N, nb_max): (kept, moving, arrival, urg differs, 0 -> > 0)
TALLY_K3 = {(5, 8, NB): (76, 45, 9, 7, 2), (9, 5, NB): (85, 53, 16, 16, 6), (70, 4, NB): (565, 363, 121, 73, 26),
            (3, 64, NB): (250, 188, 78, 32, 16), (2, 130, NB): (302, 226, 71, 56, 24), (2, 65, 200): (195, 152, 24, 23, 8)}
# (at k = 1 the set of 200 has no row going from 0 to > 0: the four other counts are asserted there)
TALLY_K1 = {(5, 8, NB): (30, 22, 4, 3, 2), (9, 5, NB): (37, 21, 8, 5, 2), (70, 4, NB): (253, 149, 40, 42, 18),
            (3, 64, NB): (110, 81, 34, 15, 7), (2, 130, NB): (125, 89, 24, 26, 7), (2, 65, 200): (65, 51, 7, 4, 0)}
TALLY_NAMES = ("kept", "moving", "arrival", "urg_differs", "zero_to_positive")


# ---- the scene (host side) --------------------------------------------------------------------------------------------------

def routes(E, N):
    wp = np.zeros((E, N, 2, 3))
    wp[:, :, 0] = [1.0, 1.0, 1.0]
    wp[:, :, 1] = [5.0, 5.0, 5.0]
    return wp, np.full((E, N), 2, np.int32)


@functools.lru_cache(maxsize=None)
def moved_scene(E, N, nb_max=NB, drone_counts=None):
    """pos, vel [E, N, 3], rad [E, N]; bld0 [E, nb_max, 4] / cnt [E]: the sets at the start; ends, speed: the patrols; bld
    (fillers with h = -inf, as the handle holds them) and leg: after MOVES moves by the numpy reference; world."""
    rng = np.random.default_rng(E * 1000 + N + 7 * nb_max)
    pos = rng.uniform(0.0, 1.0, (E, N, 3)) * np.array(MAP)
    ang, spd = rng.uniform(0, 2 * np.pi, (E, N)), rng.uniform(0.0, 2.0, (E, N))
    vel = np.stack([spd * np.cos(ang), spd * np.sin(ang), rng.uniform(-1, 1, (E, N))], axis=-1)
    vel[:, ::5] = 0.0
    rad = np.round(rng.uniform(0.1, 0.4, (E, N)), 3)
    bld0 = np.concatenate([rng.uniform(0, MAP[0], (E, nb_max, 1)), rng.uniform(0, MAP[1], (E, nb_max, 1)),
                           rng.uniform(0, MAP[2] + 2, (E, nb_max, 1)), rng.uniform(0.3, 1.5, (E, nb_max, 1))], axis=-1)
    cnt = np.full(E, nb_max - 3, dtype=np.int32)
    cnt[0], cnt[E - 1] = nb_max, 0
    bld0[0, 1], bld0[0, 2] = [4.0, 4.0, 7.0, 0.5], [4.0, 12.0, 7.0, 0.5]
    wp, n_points = routes(E, N)
    world = World(wp, n_points, np.array(MAP), bld0, cnt, None if drone_counts is None else np.array(drone_counts, np.int32))
    pat = synthetic_patrols(world, seed=E + N, speed=(0.3, 1.5), span=6.0, dt=DT, device="cpu")
    ends, speed = pat.ends.numpy().copy(), pat.speed.numpy().copy()
    speed[:, ::4] = 0.0
    speed[:, 5] = np.nan
    ends[0, 1], speed[0, 1] = [[4.0, 4.0], [16.0, 4.0]], 1.0     # after three moves at (7, 4), velocity (1, 0)
    ends[0, 2], speed[0, 2] = [[4.0, 12.0], [16.0, 12.0]], 0.5   # ... at (5.5, 12), velocity (0.5, 0)
    pos[0, 0], vel[0, 0] = [8.0, 4.0, 3.0], 0.0
    pos[0, 1], vel[0, 1] = [4.5, 12.0, 3.0], [0.5, 0.0, 0.25]
    rad[0, :2] = 0.25
    live = np.arange(nb_max)[None, :] < cnt[:, None]
    bld = bld0.copy()
    bld[~live, 2] = -np.inf
    leg = np.ones((E, nb_max), np.uint8)
    for _ in range(MOVES):
        bld, leg = mref.move(bld, ends, speed, leg, DT)
    assert bld[0, 1, :2].tolist() == [7.0, 4.0] and bld[0, 2, :2].tolist() == [5.5, 12.0]
    return types.SimpleNamespace(E=E, N=N, nb_max=nb_max, pos=pos, vel=vel, rad=rad, bld0=bld0, cnt=cnt, ends=ends, speed=speed,
                                 bld=bld, leg=leg, live=live, world=world, drone_counts=drone_counts)


@functools.lru_cache(maxsize=None)
def want(E, N, nb_max, k, moving=True, drone_counts=None):
    """The restatement on moved_scene: (rows [E, N, k, 8], b_count, tally, branch); moving=False: motion == NULL."""
    sc = moved_scene(E, N, nb_max, drone_counts)
    pos, vel = sc.pos, sc.vel
    return building_rows_moving_ref(pos, vel, sc.rad, sc.bld, k, (sc.ends, sc.speed, sc.leg) if moving else None, DT,
                                    counts=drone_counts, building_counts=sc.cnt)


def tally_of(E, N, nb_max, k):
    t = want(E, N, nb_max, k)[2]
    return tuple(int(t[n]) for n in TALLY_NAMES)


# ---- the device side ----------------------------------------------------------------------------------------------------------

def fbits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def live_env(sc, nm=NM):
    """The env of the scene with its motion attached and advanced MOVES times: the records are where the numpy reference
    has them, bit for bit."""
    env = BatchedDroneEnv(sc.world, neighbors_num=nm, radius=sc.rad)
    motion = BuildingMotion(sc.ends, sc.speed, dt=DT)
    env.attach_building_motion(motion)
    for _ in range(MOVES):
        motion.advance()
    env.set_state(pos=sc.pos, vel=sc.vel)
    got = motion.buildings.cpu().numpy()
    assert np.array_equal(got[sc.live].view(np.uint64), sc.bld[sc.live].view(np.uint64))
    assert np.array_equal(motion.leg.cpu().numpy(), sc.leg)
    return env, motion


def call(env, k, rows, row_ld, col0=0, b_count=None, obs=None, motion="attached", dt=DT, reach=5.0, below=2.0):
    """The raw entry point.  motion: "attached" (the env's), None, or a _lib.BuildingMotionArgs."""
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    a = _lib.BuildingRowsArgs(k, reach, below, p(rows), row_ld, col0, p(b_count), p(obs))
    m = motion
    if isinstance(motion, str):
        m = None if env._motion is None else env._motion._args
    return _lib.lib().rvo3d_building_rows_moving(env._h, C.byref(a), None if m is None else C.byref(m), dt, env._stream())


@pytest.mark.parametrize("E,N,nb_max", SHAPES)
def test_rows_equal_the_restatement_bit_for_bit(E, N, nb_max):
    """Stand-alone and widen mode at k = 1, 3, 8: rows, b_count, no -0.0, a second call gives the same bits; the wide row
    is cat(dense[:12], rows8, dense[12:]) and the columns behind W + 8k keep their fill."""
    sc = moved_scene(E, N, nb_max)
    env, motion = live_env(sc)
    dense = env.observe()[0].clone()
    W = env.W
    assert W == 39
    for k in (1, 3, 8):
        w_rows, w_cnt, tally, _ = want(E, N, nb_max, k)
        assert tally["moving"] > 0 and tally["kept"] > tally["moving"]
        rows, bc = env.building_rows(k, velocity=True)
        g_rows, g_cnt = rows.cpu().numpy(), bc.cpu().numpy()
        assert g_rows.shape == (E, N, k, 8) and g_cnt.dtype == np.int32
        bad = np.argwhere(fbits(g_rows) != fbits(w_rows))
        assert bad.size == 0, (k, len(bad), bad[:4].tolist(), g_rows[tuple(bad[0][:3])], w_rows[tuple(bad[0][:3])])
        assert np.array_equal(g_cnt, w_cnt), k
        assert not (np.signbit(g_rows) & (g_rows == 0)).any()   # no -0.0
        assert (g_cnt[E - 1] == 0).all() and not g_rows[E - 1].any()   # a set of 0 buildings: fillers alone
        first = rows.clone()
        rows2, _ = env.building_rows(k, velocity=True)
        assert rows2.data_ptr() == rows.data_ptr() and same(rows2, first)
        wide = torch.full((E, N, W + 8 * k + 3), -7.0, device="cuda")
        assert call(env, k, wide, W + 8 * k + 3, col0=12, obs=dense) == 0
        hand = torch.cat([dense[..., :12], first.view(E, N, 8 * k), dense[..., 12:], torch.full((E, N, 3), -7.0, device="cuda")],
                         dim=-1)
        assert same(wide, hand), k
    env.close()


@pytest.mark.parametrize("E,N,nb_max", SHAPES)
def test_cross_checks_against_the_rows_of_six(E, N, nb_max):
    """On the same state: columns 0..4 and b_count are rvo3d_building_rows' for every row; with motion == NULL column 5 is
    too and columns 6, 7 are +0.0; inside the moving set the rows of static records (speed 0, NaN) carry the static urg
    and zero velocity - and some rows of moving records do not."""
    sc = moved_scene(E, N, nb_max)
    env, motion = live_env(sc)
    for k in (1, 3, 8):
        _, _, tally, branch = want(E, N, nb_max, k)
        r6, c6 = (t.clone() for t in env.building_rows(k))
        r8, c8 = (t.clone() for t in env.building_rows(k, velocity=True))
        assert same(r8[..., :5], r6[..., :5]) and torch.equal(c8, c6), k
        null = torch.full((E, N, k, 8), -7.0, device="cuda")
        cn = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
        assert call(env, k, null, 8 * k, b_count=cn, motion=None) == 0
        assert same(null[..., :6], r6) and torch.equal(cn, c6) and not bool(null[..., 6:].view(torch.int32).any()), k
        assert call(env, k, null, 8 * k, b_count=cn, motion=None, dt=0.0) == 0 and same(null[..., :6], r6)
        static = torch.from_numpy(branch == 0).cuda()
        assert bool(static.any()) and same(r8[static][:, :6], r6[static]) and not bool(r8[static][:, 6:].view(torch.int32).any()), k
        moving = torch.from_numpy(branch > 0).cuda()
        differs = int((r8[..., 5] != r6[..., 5]).sum())
        assert differs == tally["urg_differs"] and not bool((r8[..., 5] != r6[..., 5])[~moving].any()), (k, differs)
        assert int(((r6[..., 5] == 0) & (r8[..., 5] > 0)).sum()) == tally["zero_to_positive"], k
        assert bool(r8[moving][:, 6:].any()) and differs > 0
    env.close()


@pytest.mark.parametrize("E,N,nb_max", SHAPES)
def test_the_scene_is_not_vacuous(E, N, nb_max):
    """Per shape, from the restatement: among the kept rows at least one moving building, one on the arrival branch, one
    whose r2(urg_rel) differs from the static r2(urg), one going from 0 to > 0 (at k = 3; at k = 1 the first three) - the
    counts of the module docstring - and
    the device's rows show the same counts.  The planted pairs of env 0, in the k = 8 rows of the device."""
    sc = moved_scene(E, N, nb_max)
    for k, table in ((3, TALLY_K3), (1, TALLY_K1)):
        got = tally_of(E, N, nb_max, k)
        print((E, N, nb_max), "k", k, dict(zip(TALLY_NAMES, got)))
        assert got == table[E, N, nb_max], (k, got)
        assert min(got if k == 3 else got[:4]) >= 1, (k, got)
    env, motion = live_env(sc)
    for k in (3, 1):
        _, _, tally, branch = want(E, N, nb_max, k)
        r6 = env.building_rows(k)[0].clone()
        r8 = env.building_rows(k, velocity=True)[0]
        assert int((r8[..., 5] != r6[..., 5]).sum()) == tally["urg_differs"]
        assert int(((r6[..., 5] == 0) & (r8[..., 5] > 0)).sum()) == tally["zero_to_positive"]
    # the arrival branch as the device sees it: the row's velocity is the way to the endpoint over dt, not the speed
    _, _, _, branch = want(E, N, nb_max, 8)
    r8, c8 = (t.cpu().numpy() for t in env.building_rows(8, velocity=True))
    r6 = env.building_rows(8)[0].cpu().numpy()
    assert (branch == 1).any() and (branch == 2).any()
    speed_of_row = np.hypot(r8[..., 6].astype(np.float64), r8[..., 7].astype(np.float64))
    assert (speed_of_row[branch == 2] >= 0.29).all() and (speed_of_row[branch == 1] < 1.52).all()

    def slot_of(d, b_xy):
        w = np.float32(np.round(np.asarray(b_xy) - sc.pos[0, d, :2], 2))
        hits = [s for s in range(c8[0, d]) if np.array_equal(r8[0, d, s, :2], w)]
        assert len(hits) == 1, (d, hits)
        return hits[0]
    s = slot_of(0, (7.0, 4.0))       # the standing drone, record 1 coming at it: 1 m - 0.75 m at 1 m per step -> 1 / 0.45
    assert r6[0, 0, s, 5] == 0 and r8[0, 0, s, 5] == np.float32(2.22) and r8[0, 0, s, 6:].tolist() == [1.0, 0.0]
    s = slot_of(1, (5.5, 12.0))      # the drone behind record 2 at record 2's velocity: 0.25 m at 0.5 m per step -> 1 / 0.7
    assert r6[0, 1, s, 5] == np.float32(1.43) and r8[0, 1, s, 5] == 0 and r8[0, 1, s, 6:].tolist() == [0.5, 0.0]
    env.close()


@pytest.mark.parametrize("E,N", [(5, 8), (2, 130)])
def test_widen_mode_at_an_even_width(E, N):
    """neighbors_num = 10: W = 102, wide rows of 110 / 126 / 166 floats, row_ld = W + 8k exactly: the row behind starts
    where this one ends.  One poisoned guard row before and one behind stay as they were."""
    sc = moved_scene(E, N, NB)
    env, motion = live_env(sc, nm=10)
    dense = env.observe()[0].clone()
    W = env.W
    assert W == 102
    for k in (1, 3, 8):
        w_rows = want(E, N, NB, k)[0]
        ld = W + 8 * k
        buf = torch.full((E * N + 2, ld), -7.0, device="cuda")
        assert call(env, k, buf[1:], ld, col0=12, obs=dense) == 0
        hand = torch.cat([dense[..., :12], torch.from_numpy(w_rows).cuda().view(E, N, 8 * k), dense[..., 12:]], dim=-1)
        assert same(buf[1:-1], hand.view(E * N, ld)), k
        assert bool((buf[0] == -7).all()) and bool((buf[-1] == -7).all()), k
    env.close()


COUNTED = [(4, 130, (130, 65, 64, 1)), (70, 4, tuple((4, 1, 3, 2)[e % 4] for e in range(70)))]


@pytest.mark.parametrize("E,N,counts", COUNTED)
def test_counted_handle_ghost_rows(E, N, counts):
    """A counted handle (three waves per env with waves of ghosts alone; the packed geometry with a second workgroup) with
    NaN in the ghosts' state, into pre-filled outputs: live rows equal the restatement, ghost rows and their b_count are
    zeros, and a ghost's whole wide row is zeros although the dense obs handed in holds a poison value there."""
    sc = moved_scene(E, N, NB, counts)
    cn = np.array(counts)
    ghost = np.arange(N)[None, :] >= cn[:, None]
    assert ghost.any() and (~ghost).any()
    env, motion = live_env(sc)
    pos_g, vel_g = sc.pos.copy(), sc.vel.copy()
    pos_g[ghost], vel_g[ghost] = np.nan, np.nan
    env.set_state(pos=pos_g, vel=vel_g)
    dense = env.observe()[0].clone()
    g = torch.from_numpy(ghost).cuda()
    assert not bool(dense[g].any())
    live_dense = dense.clone()
    dense[g] = -7.0
    W = env.W
    for k in (1, 3, 8):
        w_rows, w_cnt, tally, _ = want(E, N, NB, k, True, counts)
        assert w_rows[~ghost].any() and not w_rows[ghost].any() and tally["urg_differs"] > 0
        rows = torch.full((E, N, k, 8), -7.0, device="cuda")
        bc = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
        assert call(env, k, rows, 8 * k, b_count=bc) == 0
        bad = np.argwhere(fbits(rows.cpu().numpy()) != fbits(w_rows))
        assert bad.size == 0, (k, len(bad), bad[:4].tolist())
        assert np.array_equal(bc.cpu().numpy(), w_cnt) and not bc.cpu().numpy()[ghost].any(), k
        wide = torch.full((E, N, W + 8 * k), -7.0, device="cuda")
        assert call(env, k, wide, W + 8 * k, col0=12, obs=dense) == 0
        hand = torch.cat([live_dense[..., :12], torch.from_numpy(w_rows).cuda().view(E, N, 8 * k), live_dense[..., 12:]], dim=-1)
        assert same(wide, hand), k
        assert not wide.cpu().numpy()[ghost].view(np.uint8).any(), k
    env.close()


def test_shared_list_and_stand_alone_columns():
    """motion == NULL is allowed on a handle of the shared list; in a wider buffer every column outside
    [col0, col0 + 8k) and the guard rows stay as they were."""
    E, N, k, ld, col0 = 5, 8, 3, 41, 7
    sc = moved_scene(E, N, NB)
    wp, n_points = routes(E, N)
    shared = sc.bld[0]
    env = BatchedDroneEnv(World(wp, n_points, np.array(MAP), shared, None, None), neighbors_num=NM, radius=sc.rad)
    env.set_state(pos=sc.pos, vel=sc.vel)
    w_rows, w_cnt, _, _ = building_rows_moving_ref(sc.pos, sc.vel, sc.rad, shared, k)
    assert w_rows.any()
    buf = torch.full((E * N + 2, ld), -7.0, device="cuda")
    assert call(env, k, buf[1:], ld, col0=col0) == 0
    got = buf.cpu().numpy()
    assert np.array_equal(fbits(got[1:-1, col0:col0 + 8 * k]), fbits(w_rows.reshape(E * N, 8 * k)))
    assert (got[0] == -7).all() and (got[-1] == -7).all()
    assert (got[:, :col0] == -7).all() and (got[:, col0 + 8 * k:] == -7).all()
    rows, bc = env.building_rows(k, velocity=True)   # the Python surface without a motion
    r6, _ = env.building_rows(k)
    assert same(rows[..., :6], r6) and not bool(rows[..., 6:].view(torch.int32).any()) and np.array_equal(bc.cpu().numpy(), w_cnt)
    env.close()


def test_refused_calls_write_nothing():
    E, N, k = 5, 8, 3
    sc = moved_scene(E, N, NB)
    env, motion = live_env(sc)
    dense = env.observe()[0].clone()
    W = env.W
    ld = W + 64
    rows = torch.full((E, N, ld), -7.0, device="cuda")
    bc = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    ok = motion._args
    ptrs = [motion.ends.data_ptr(), motion.speed.data_ptr(), motion.leg.data_ptr()]
    INVALID, STATE = -1, -3
    bad = [(dict(row_ld=8 * k - 1), INVALID, b"8 * k"), (dict(col0=5, row_ld=5 + 8 * k - 1), INVALID, b"8 * k"),
           (dict(row_ld=6 * k), INVALID, b"8 * k"),
           (dict(col0=0, obs=dense), INVALID, b"col0 == 12"), (dict(col0=13, obs=dense), INVALID, b"col0 == 12"),
           (dict(col0=12, obs=dense, row_ld=W + 8 * k - 1), INVALID, b"8 * k"),
           (dict(col0=12, obs=rows), INVALID, b"overlap"), (dict(col0=12, obs=rows.view(-1)[W:]), INVALID, b"overlap"),
           (dict(k=0), INVALID, b"1..8"), (dict(k=9), INVALID, b"1..8"),
           (dict(dt=-1.0), INVALID, b"dt"), (dict(dt=float("inf")), INVALID, b"dt"), (dict(dt=float("nan")), INVALID, b"dt"),
           (dict(dt=-1.0, motion=None), INVALID, b"dt")]
    for j, name in enumerate(("ends", "speed", "leg")):
        p = list(ptrs)
        p[j] = None
        bad.append((dict(motion=_lib.BuildingMotionArgs(*p)), INVALID, b"required"))
    for kw, code, text in bad:
        a = dict(k=k, rows=rows, row_ld=ld, col0=0, b_count=bc, obs=None)
        a.update(kw)
        rc = call(env, a.pop("k"), a.pop("rows"), a.pop("row_ld"), **a)
        assert rc == code and text in L.rvo3d_last_error(), (kw, rc, L.rvo3d_last_error())
    # a motion without attached sets: a handle of the shared list
    wp, n_points = routes(E, N)
    shared = BatchedDroneEnv(World(wp, n_points, np.array(MAP), sc.bld[0], None, None), neighbors_num=NM, radius=sc.rad)
    shared.set_state(pos=sc.pos, vel=sc.vel)
    assert call(shared, k, rows, ld, b_count=bc, motion=ok) == STATE and b"rvo3d_set_env_buildings" in L.rvo3d_last_error()
    # a handle without a world, no handle
    h = C.c_void_p()
    cfg = _lib.Config(E, N, 2, 0, NM, 1, 0, -1, (C.c_double * 3)(*MAP))
    assert L.rvo3d_create(C.byref(cfg), C.byref(h)) == 0
    a = _lib.BuildingRowsArgs(k, 5.0, 2.0, rows.data_ptr(), ld, 0, None, None)
    assert L.rvo3d_building_rows_moving(h, C.byref(a), None, 1.0, None) == STATE and b"rvo3d_load_world" in L.rvo3d_last_error()
    assert L.rvo3d_building_rows_moving(None, C.byref(a), None, 1.0, None) == INVALID
    L.rvo3d_destroy(h)
    torch.cuda.synchronize()
    assert bool((rows == -7).all()) and bool((bc == -7).all())
    assert bool((motion.leg.cpu() == torch.from_numpy(sc.leg)).all())
    # ... and the same buffers are fine when asked properly
    assert call(env, k, rows, ld, col0=12, b_count=bc, obs=dense) == 0
    assert bool((bc >= 0).all()) and bool((rows[..., W + 8 * k:] == -7).all())
    with pytest.raises(_lib.RVO3DError):
        env.building_rows(9, velocity=True)
    shared.close()
    env.close()
