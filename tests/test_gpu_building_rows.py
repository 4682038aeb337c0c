"""Nearest-building rows on the device (include/rvo3d.h: rvo3d_building_rows) against the plain-Python restatement
(tests/building_rows_ref.py), bit for bit, over the launch geometries and building set-ups; the two output modes, what
they leave alone, and the argument contract.  The shapes and why each is there stand next to SHAPES; further cases:
building lists that end one record before, on and one record behind a tile boundary; widen mode at the even width
W = 102; counted handles beyond one wave, with waves made of ghosts alone, per-env sets, and in the packed geometry."""
import ctypes as C

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, World, _lib
from building_rows_ref import building_rows_ref, drone_rows

pytestmark = pytest.mark.gpu
MAP = (20.0, 16.0, 8.0)
NM = 3   # W = 39: odd, so are the wide rows of even 6k - rows that are only 4-byte aligned
# (E, N, buildings): the packed geometry with three building tiles of 8; a full wave per env; two waves; per-env sets of
# 200 records (two tiles of 192) whose counts include 0 and 200, the unused records padded with h = -inf by the library;
# then the launch geometry's other corners:
#   (70, 4)   L = 4, 64 envs per workgroup: a second workgroup (blockIdx.x > 0) that is partly filled, shared and per-env
#   (9, 5)    L = 8 > N: padding lanes inside every env's lane group (l >= N; the row writer's ql >= N), two workgroups
#   (7, 33)   L = 64 > N: 31 padding lanes per wave
#   (2, 257)  T = 320: five waves share the row writer, three staging batches of kBldStage (128 + 128 + 64)
#   (1, 512)  T = 512: eight waves, four full staging batches
# and, in a test of their own, (5, 1) and (3, 2): L = 1 and L = 2.
SHAPES = [(5, 8, "shared"), (3, 64, "shared"), (2, 65, "shared"), (2, 130, "per_env"),
          (70, 4, "shared"), (9, 5, "shared"), (7, 33, "shared"), (2, 257, "shared"), (1, 512, "shared"), (70, 4, "per_env")]
SMALL_FLEETS = [(5, 1), (3, 2)]


def fbits(a):
    return np.ascontiguousarray(a).view(np.int32)


def scene(E, N, kind, seed):
    """Random drones in the map, speeds up to 2, and in env 0 the planted ones next to the planted buildings 0..2:
      d0 offset (3, 4) from building 0: d == 5.0 exactly, passes;  d1 at p_z == h_0 + 2 exactly: building 0 fails;
      d2 inside building 0's cylinder: urg = 5;  d3 standing still between buildings 1 and 2, at equal gaps: urg = 0, the
      lower index first;  d4 flying straight at building 1."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 1.0, (E, N, 3)) * np.array(MAP)
    ang, spd = rng.uniform(0, 2 * np.pi, (E, N)), rng.uniform(0.0, 2.0, (E, N))
    vel = np.stack([spd * np.cos(ang), spd * np.sin(ang), rng.uniform(-1, 1, (E, N))], axis=-1)
    vel[:, ::5] = 0.0
    rad = np.round(rng.uniform(0.1, 0.4, (E, N)), 3)
    planted = np.array([[10.0, 6.0, 6.0, 1.0], [4.0, 12.0, 7.0, 0.5], [8.0, 12.0, 7.0, 0.5]])

    m = 0.0 if kind == "shared" else 1.0   # the sets of 200 spread over nine times the map: some drones see few of them

    def draw(*shape):
        return np.concatenate([rng.uniform(-m * MAP[0], (1 + m) * MAP[0], shape + (1,)),
                               rng.uniform(-m * MAP[1], (1 + m) * MAP[1], shape + (1,)),
                               rng.uniform(0, MAP[2] + 2, shape + (1,)), rng.uniform(0.3, 1.5, shape + (1,))], axis=-1)
    if kind == "shared":
        bld, cnt = draw(20), None
        bld[:3] = planted
    else:
        bld = draw(E, 200)
        bld[:, :3] = planted
        cnt = np.full(E, 117, dtype=np.int32)
        cnt[0], cnt[E - 1] = 200, 0
    pos[0, 0] = [13.0, 10.0, 3.0]; vel[0, 0] = [-0.75, -1.0, 0.25]
    pos[0, 1] = [9.0, 3.0, 8.0]; vel[0, 1] = [0.5, 0.5, 0.0]
    pos[0, 2] = [10.25, 6.125, 3.0]; vel[0, 2] = [1.0, 0.0, 0.0]
    pos[0, 3] = [6.0, 12.0, 3.0]; vel[0, 3] = 0.0
    pos[0, 4] = [0.5, 12.0, 5.0]; vel[0, 4] = [1.5, 0.0, 0.0]
    rad[0, :5] = 0.25
    return pos, vel, rad, bld, cnt


def scene_cut(E, N, kind, seed):
    """scene() for fleets below its five planted drones: the scene of five with the first N drones kept."""
    pos, vel, rad, bld, cnt = scene(E, max(N, 5), kind, seed)
    return pos[:, :N].copy(), vel[:, :N].copy(), rad[:, :N].copy(), bld, cnt


def check_planted(r8, c8, pos):
    """The planted drones of env 0 in the k = 8 rows (scene)."""
    def slot_of(d, b_xy):
        want = np.float32(np.round(np.asarray(b_xy) - pos[0, d, :2], 2))
        hits = [s for s in range(c8[0, d]) if np.array_equal(r8[0, d, s, :2], want)]
        return hits[0] if hits else None
    assert slot_of(0, (10.0, 6.0)) is not None          # d == 5.0 passes
    assert slot_of(1, (10.0, 6.0)) is None              # h_b == p_z - 2 fails
    s = slot_of(2, (10.0, 6.0))
    assert s is not None and r8[0, 2, s, 5] == 5.0 and r8[0, 2, s, 4] < 0     # inside the cylinder: urg = 5
    s1, s2 = slot_of(3, (4.0, 12.0)), slot_of(3, (8.0, 12.0))
    assert s1 is not None and s2 == s1 + 1              # equal gaps: building 1 right before building 2
    assert r8[0, 3, s1, 4] == r8[0, 3, s2, 4] == 1.25 and r8[0, 3, s1, 5] == r8[0, 3, s2, 5] == 0   # standing still
    s = slot_of(4, (4.0, 12.0))
    assert s is not None and 0 < r8[0, 4, s, 5] < 5.0   # on its way there


def make_env(E, N, bld, cnt, rad, drone_counts=None, nm=NM):
    wp = np.zeros((E, N, 2, 3))
    wp[:, :, 0] = [1.0, 1.0, 1.0]
    wp[:, :, 1] = [5.0, 5.0, 5.0]
    w = World(wp, np.full((E, N), 2, np.int32), np.array(MAP), bld, cnt, drone_counts)
    return BatchedDroneEnv(w, neighbors_num=nm, radius=rad)


def call(env, k, rows, row_ld, col0=0, b_count=None, obs=None, reach=5.0, below=2.0):
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    a = _lib.BuildingRowsArgs(k, reach, below, p(rows), row_ld, col0, p(b_count), p(obs))
    return _lib.lib().rvo3d_building_rows(env._h, C.byref(a), env._stream())


def state_bits(env):
    return {k: v.cpu().numpy().copy() for k, v in env.get_state().items()}


def rows_against_the_restatement(E, N, kind, enough):
    """Stand-alone and widen mode at k = 1, 4, 8 against building_rows_ref; enough(k, kind, passing): the scene's
    own non-vacuity condition."""
    pos, vel, rad, bld, cnt = scene_cut(E, N, kind, seed=E * 1000 + N)
    env = make_env(E, N, bld, cnt, rad)
    env.set_state(pos=pos, vel=vel)
    dense = env.observe()[0].clone()
    before = state_bits(env)
    W = env.W
    for k in (1, 4, 8):
        w_rows, w_cnt, passing = building_rows_ref(pos, vel, rad, bld, k, building_counts=cnt)
        rows, bc = env.building_rows(k)
        g_rows, g_cnt = rows.cpu().numpy(), bc.cpu().numpy()
        assert g_rows.shape == (E, N, k, 6) and g_cnt.dtype == np.int32
        bad = np.argwhere(fbits(g_rows) != fbits(w_rows))
        assert bad.size == 0, (k, bad[:4].tolist(), g_rows[tuple(bad[0][:2])], w_rows[tuple(bad[0][:2])])
        assert np.array_equal(g_cnt, w_cnt), k
        assert not (np.signbit(g_rows) & (g_rows == 0)).any()   # no -0.0
        enough(k, kind, passing)
        if kind == "per_env":
            assert (g_cnt[E - 1] == 0).all() and not g_rows[E - 1].any()   # a set of 0 buildings: padding alone
        # a second call: the same bits
        first = rows.clone()
        rows2, _ = env.building_rows(k)
        assert rows2.data_ptr() == rows.data_ptr() and torch.equal(rows2.view(torch.int32), first.view(torch.int32))
        # widen mode == torch.cat of the dense observation and the stand-alone rows; columns behind W + 6k stay
        wide = torch.full((E, N, W + 6 * k + 3), -7.0, device="cuda")
        assert call(env, k, wide, W + 6 * k + 3, col0=12, obs=dense) == 0
        want = torch.cat([dense[..., :12], first.view(E, N, 6 * k), dense[..., 12:],
                          torch.full((E, N, 3), -7.0, device="cuda")], dim=-1)
        assert torch.equal(wide.view(torch.int32), want.view(torch.int32)), k
    # the planted cases are what they were planted for
    r8, c8 = (t.cpu().numpy() for t in env.building_rows(8))
    if kind == "shared" and N >= 5:
        check_planted(r8, c8, pos)
    # no state array was touched
    after = state_bits(env)
    for name in before:
        assert np.array_equal(before[name].view(np.uint8), after[name].view(np.uint8)), name
    env.close()


@pytest.mark.parametrize("E,N,kind", SHAPES)
def test_rows_equal_the_restatement_bit_for_bit(E, N, kind):
    def enough(k, kind, passing):
        assert (passing > k).any() or (k == 8 and kind == "shared")
        assert ((passing > 0) & (passing < k)).any() or k == 1
    rows_against_the_restatement(E, N, kind, enough)


@pytest.mark.parametrize("E,N", SMALL_FLEETS)
def test_rows_of_fleets_of_one_and_two(E, N):
    """One and two lanes per env.  At (5, 1) no drone has more than four passing buildings and every drone has one, so
    the condition here is: some drone sees a building, and some drone fewer than k (k = 1 left out, as above)."""
    def enough(k, kind, passing):
        assert (passing > 0).any() and ((passing < k).any() or k == 1)
    rows_against_the_restatement(E, N, "shared", enough)


def boundary_list():
    """129 records drawn as scene() draws a shared list; the lists of the boundary test are its first nb."""
    rng = np.random.default_rng(129)
    b = np.stack([rng.uniform(0, MAP[0], 129), rng.uniform(0, MAP[1], 129), rng.uniform(0, MAP[2] + 2, 129),
                  rng.uniform(0.3, 1.5, 129)], axis=-1)
    b[:3] = [[10.0, 6.0, 6.0, 1.0], [4.0, 12.0, 7.0, 0.5], [8.0, 12.0, 7.0, 0.5]]
    return b


@pytest.mark.parametrize("E,N,nb", [(5, 8, 7), (5, 8, 8), (5, 8, 9), (2, 65, 127), (2, 65, 128), (2, 65, 129)])
def test_list_ends_on_a_tile_boundary(E, N, nb):
    """nb == L - 1, L, L + 1 (L = 8 lanes per env at N = 8, 128 at N = 65): the last tile is one record short, full, or
    a single record.  In env 1 a drone stands 0.3 m from each of the records 6..8 / 126..128, so that the list's last
    record is kept in somebody's k = 8 rows; the three lists differ in their tail only."""
    k = 8
    pos, vel, rad, _, _ = scene(E, N, "shared", seed=E * 1000 + N)
    full = boundary_list()
    L = 8 if N == 8 else 128
    for i, b in enumerate(full[L - 2:L + 1]):
        pos[1, i] = [b[0] + b[3] + rad[1, i] + 0.3, b[1], b[2]]
    bld = full[:nb].copy()
    assert nb in (L - 1, L, L + 1)
    w_rows, w_cnt, _ = building_rows_ref(pos, vel, rad, bld, k)
    kept_by = [(e, d) for e in range(E) for d in range(N) if nb - 1 in drone_rows(pos[e, d], vel[e, d], rad[e, d], bld, k)[2]]
    assert kept_by, "the last record is in nobody's rows"
    env = make_env(E, N, bld, None, rad)
    env.set_state(pos=pos, vel=vel)
    rows, bc = env.building_rows(k)
    g_rows, g_cnt = rows.cpu().numpy(), bc.cpu().numpy()
    bad = np.argwhere(fbits(g_rows) != fbits(w_rows))
    print(f"({E}, {N}), nb {nb}: rows that keep the last record {len(kept_by)}, mismatching floats {len(bad)}")
    assert bad.size == 0, (bad[:4].tolist(), g_rows[tuple(bad[0][:2])], w_rows[tuple(bad[0][:2])])
    assert np.array_equal(g_cnt, w_cnt)
    env.close()


@pytest.mark.parametrize("E,N,kind", [(5, 8, "shared"), (2, 130, "per_env")])
def test_widen_mode_at_an_even_width(E, N, kind):
    """neighbors_num = 10: W = 102, wide rows of 108 / 126 / 150 floats whose starts are 16- or 8-byte aligned (W = 39
    gives 4-byte alignment only), row_ld = W + 6k exactly: the row behind starts where this one ends.  One poisoned
    guard row before and one behind stay as they were."""
    pos, vel, rad, bld, cnt = scene(E, N, kind, seed=E * 1000 + N)
    env = make_env(E, N, bld, cnt, rad, nm=10)
    env.set_state(pos=pos, vel=vel)
    dense = env.observe()[0].clone()
    W = env.W
    assert W == 102
    for k in (1, 4, 8):
        w_rows, _, passing = building_rows_ref(pos, vel, rad, bld, k, building_counts=cnt)
        assert (passing > 0).any()
        ld = W + 6 * k
        buf = torch.full((E * N + 2, ld), -7.0, device="cuda")
        assert buf[1:].data_ptr() % 8 == 0
        assert call(env, k, buf[1:], ld, col0=12, obs=dense) == 0
        want = torch.cat([dense[..., :12], torch.from_numpy(w_rows).cuda().view(E, N, 6 * k), dense[..., 12:]], dim=-1)
        assert torch.equal(buf[1:-1].view(torch.int32), want.view(E * N, ld).view(torch.int32)), k
        assert bool((buf[0] == -7).all()) and bool((buf[-1] == -7).all()), k
    env.close()


def counted_case(E, N, kind, counts, building_counts=None):
    """A counted handle with NaN in the ghosts' position and velocity, into pre-filled outputs in both modes: live rows
    equal the restatement, ghost rows and ghost b_count are zeros, and a ghost's whole wide row is zeros although the
    dense obs handed in holds a poison value there."""
    pos, vel, rad, bld, cnt = scene_cut(E, N, kind, seed=E * 1000 + N + 1)
    cnt = cnt if building_counts is None else np.array(building_counts, dtype=np.int32)
    counts = np.array(counts, dtype=np.int32)
    env = make_env(E, N, bld, cnt, rad, drone_counts=counts)
    ghost = np.arange(N)[None, :] >= counts[:, None]
    assert ghost.any() and (~ghost).any()
    pos_g, vel_g = pos.copy(), vel.copy()
    pos_g[ghost], vel_g[ghost] = np.nan, np.nan
    env.set_state(pos=pos_g, vel=vel_g)
    dense = env.observe()[0].clone()
    g = torch.from_numpy(ghost).cuda()
    assert not bool(dense[g].any())
    live_dense = dense.clone()
    dense[g] = -7.0
    W = env.W
    for k in (1, 4, 8):
        w_rows, w_cnt, passing = building_rows_ref(pos_g, vel_g, rad, bld, k, counts=counts, building_counts=cnt)
        assert w_rows[~ghost].any() and not w_rows[ghost].any() and (passing > 0).any()
        rows = torch.full((E, N, k, 6), -7.0, device="cuda")
        bc = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
        assert call(env, k, rows, 6 * k, b_count=bc) == 0
        bad = np.argwhere(fbits(rows.cpu().numpy()) != fbits(w_rows))
        assert bad.size == 0, (k, len(bad), bad[:4].tolist())
        assert np.array_equal(bc.cpu().numpy(), w_cnt) and not bc.cpu().numpy()[ghost].any(), k
        wide = torch.full((E, N, W + 6 * k), -7.0, device="cuda")
        assert call(env, k, wide, W + 6 * k, col0=12, obs=dense) == 0
        want = torch.cat([live_dense[..., :12], torch.from_numpy(w_rows).cuda().view(E, N, 6 * k), live_dense[..., 12:]],
                         dim=-1)
        assert torch.equal(wide.view(torch.int32), want.view(torch.int32)), k
        assert not wide.cpu().numpy()[ghost].view(np.uint8).any(), k
    env.close()


def test_counted_handle_of_several_waves_and_per_env_sets():
    """(4, 130), three waves per env: counts 130, 65 (a wave of one live lane, a wave of ghosts), 64 (two waves of
    ghosts), 1; per-env sets of 200 records with 200, 117, 0 and 117 buildings."""
    counted_case(4, 130, "per_env", (130, 65, 64, 1), (200, 117, 0, 117))


def test_counted_handle_in_the_packed_geometry():
    """(70, 4), 64 envs per workgroup and a second, partly filled one: counts cycling 4, 1, 3, 2."""
    counted_case(70, 4, "shared", [(4, 1, 3, 2)[e % 4] for e in range(70)])


def test_counted_handle_ghost_rows():
    E, N, k = 4, 8, 4
    pos, vel, rad, bld, cnt = scene(E, N, "shared", seed=77)
    counts = np.array([1, 3, 8, 8], dtype=np.int32)
    env = make_env(E, N, bld, cnt, rad, drone_counts=counts)
    ghost = np.arange(N)[None, :] >= counts[:, None]
    pos_g, vel_g = pos.copy(), vel.copy()
    pos_g[ghost], vel_g[ghost] = np.nan, np.nan   # the ghost state is not read
    env.set_state(pos=pos_g, vel=vel_g)
    dense = env.observe()[0].clone()
    w_rows, w_cnt, _ = building_rows_ref(pos, vel, rad, bld, k, counts=counts)
    assert w_rows[~ghost].any() and not w_rows[ghost].any()
    # into pre-filled buffers: ghost rows are written as zeros, not skipped
    rows = torch.full((E, N, k, 6), -7.0, device="cuda")
    bc = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
    assert call(env, k, rows, 6 * k, b_count=bc) == 0
    assert np.array_equal(fbits(rows.cpu().numpy()), fbits(w_rows)) and np.array_equal(bc.cpu().numpy(), w_cnt)
    wide = torch.full((E, N, env.W + 6 * k), -7.0, device="cuda")
    assert call(env, k, wide, env.W + 6 * k, col0=12, obs=dense) == 0
    want = torch.cat([dense[..., :12], rows.view(E, N, 6 * k), dense[..., 12:]], dim=-1)
    assert torch.equal(wide.view(torch.int32), want.view(torch.int32))
    assert not wide.cpu().numpy()[ghost].any()   # the whole wide row of a ghost is zeros
    env.close()


def test_world_without_buildings():
    E, N = 3, 8
    pos, vel, rad, _, _ = scene(E, N, "shared", seed=5)
    env = make_env(E, N, np.zeros((0, 4)), None, rad)
    env.set_state(pos=pos, vel=vel)
    rows = torch.full((E, N, 4, 6), -7.0, device="cuda")
    bc = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
    assert call(env, 4, rows, 24, b_count=bc) == 0
    assert not rows.cpu().numpy().any() and not bc.cpu().numpy().any()
    env.close()


def test_standalone_mode_writes_its_columns_only():
    """In a wider buffer every column outside [col0, col0 + 6k) and the guard rows before and behind stay as they were;
    b_count is optional."""
    E, N, k, ld, col0 = 5, 8, 4, 41, 7
    pos, vel, rad, bld, cnt = scene(E, N, "shared", seed=9)
    env = make_env(E, N, bld, cnt, rad)
    env.set_state(pos=pos, vel=vel)
    buf = torch.full((E * N + 2, ld), -7.0, device="cuda")
    assert call(env, k, buf[1:], ld, col0=col0) == 0
    got = buf.cpu().numpy()
    w_rows, _, _ = building_rows_ref(pos, vel, rad, bld, k)
    assert np.array_equal(fbits(got[1:-1, col0:col0 + 6 * k]), fbits(w_rows.reshape(E * N, 6 * k)))
    assert (got[0] == -7).all() and (got[-1] == -7).all()
    assert (got[:, :col0] == -7).all() and (got[:, col0 + 6 * k:] == -7).all()
    env.close()


def test_refused_calls_write_nothing():
    E, N, k = 5, 8, 4
    pos, vel, rad, bld, cnt = scene(E, N, "shared", seed=9)
    env = make_env(E, N, bld, cnt, rad)
    env.set_state(pos=pos, vel=vel)
    dense = env.observe()[0].clone()
    W = env.W
    rows = torch.full((E, N, W + 48), -7.0, device="cuda")
    bc = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
    ld = W + 48
    bad = [dict(k=0), dict(k=9), dict(reach=0.0), dict(reach=-1.0), dict(reach=float("nan")), dict(reach=float("inf")),
           dict(below=-0.5), dict(below=float("nan")), dict(rows=None), dict(row_ld=6 * k - 1),
           dict(col0=5, row_ld=5 + 6 * k - 1), dict(col0=0, obs=dense), dict(col0=13, obs=dense),
           dict(col0=12, obs=dense, row_ld=W + 6 * k - 1), dict(col0=12, obs=rows), dict(col0=12, obs=rows.view(-1)[W:])]
    for kw in bad:
        a = dict(k=k, rows=rows, row_ld=ld, col0=0, b_count=bc, obs=None)
        a.update(kw)
        rc = call(env, a.pop("k"), a.pop("rows"), a.pop("row_ld"), **a)
        assert rc == -1, (kw, rc)
        assert len(_lib.lib().rvo3d_last_error()) > 0
    torch.cuda.synchronize()
    assert (rows == -7).all() and (bc == -7).all()
    assert call(env, k, rows, ld, col0=12, b_count=bc, obs=dense) == 0   # ... and the same buffers are fine when asked properly
    assert (bc >= 0).all()
    # through the Python surface
    with pytest.raises(_lib.RVO3DError):
        env.building_rows(9)
    with pytest.raises(_lib.RVO3DError):
        env.building_rows(4, reach=0.0)
    env.close()
    # a handle without a world
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _lib.Config(2, 8, 2, 0, NM, 1, 0, -1, (C.c_double * 3)(*MAP))
    assert L.rvo3d_create(C.byref(cfg), C.byref(h)) == 0
    a = _lib.BuildingRowsArgs(k, 5.0, 2.0, rows.data_ptr(), ld, 0, None, None)
    before = rows.clone()
    assert L.rvo3d_building_rows(h, C.byref(a), None) == -3   # RVO3D_ERR_STATE
    assert L.rvo3d_building_rows(None, C.byref(a), None) == -1
    torch.cuda.synchronize()
    assert torch.equal(rows.view(torch.int32), before.view(torch.int32))
    L.rvo3d_destroy(h)
