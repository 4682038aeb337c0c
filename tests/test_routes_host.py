"""The route sampler's numpy restatement (rvo3d_amd.routes.RouteSampler.sample_numpy) on the CPU: its Philox against the
published known answers, determinism, independence of the batch size, and the properties the rules promise.  The device
kernel is compared with this restatement bit for bit in tests/test_gpu_routes.py; the cases of that comparison are pinned
here by their counts, so that a misreading of the rules shows before any GPU run."""
import numpy as np
import pytest

import philox_ref
from rvo3d_amd.routes import RouteSampler, philox4x32

# (envs, drones, map, min_sep, min_len, max_tries): the cases of the device comparison
CASES = [(5, 8, (20.0, 20.0, 8.0), 3.0, 8.0, 32),
         (3, 64, (20.0, 20.0, 8.0), 2.0, 6.0, 32),
         (2, 100, (24.0, 24.0, 8.0), 1.5, 6.0, 32),
         (2, 256, (40.0, 40.0, 10.0), 1.5, 10.0, 32),
         (3, 64, (20.0, 20.0, 8.0), 2.0, 6.0, 4)]


def sampler(case, **kw):
    _, _, size, sep, length, tries = case
    return RouteSampler(size, min_sep=sep, min_len=length, margin=1.0, max_tries=tries, seed=41, **kw)


def test_philox_known_answers():
    for counter, key, want in philox_ref.KNOWN_ANSWERS:
        assert tuple(int(x) for x in philox4x32(counter, key)) == want
    # ... and as arrays, against the test suite's own implementation
    c = [np.arange(7, dtype=np.uint64) * np.uint64(k + 3) for k in range(4)]
    for a, b in zip(philox4x32(c, (5, 0xFFFFFFFF)), philox_ref.philox4x32(c, (5, 0xFFFFFFFF))):
        assert np.array_equal(a, b)


def test_counts_of_the_device_cases():
    """seed 41, draw 1, margin 1.  Drones left unplaced / starts, ends still unplaced after round 0 / last round run:

        5 x 8     map 20, 20, 8    min_sep 3.0  min_len 8.0    0    5 / 16     4
        3 x 64    map 20, 20, 8    min_sep 2.0  min_len 6.0    0   54 / 86    18
        2 x 100   map 24, 24, 8    min_sep 1.5  min_len 6.0    0   30 / 60     9
        2 x 256   map 40, 40, 10   min_sep 1.5  min_len 10.0   0   58 / 125    5
        3 x 64, max_tries 4 (second row otherwise): 10 starts + 24 ends unplaced
    """
    want = [(0, [5, 16], 4), (0, [54, 86], 18), (0, [30, 60], 9), (0, [58, 125], 5)]
    for case, (unplaced, after0, last) in zip(CASES, want):
        stats = {}
        _, _, unp = sampler(case).sample_numpy(case[0], case[1], 2, 1, stats)
        assert int(unp.sum()) == unplaced and stats["after0"] == after0 and stats["last_round"] == last, (case, stats)
    stats = {}
    _, _, unp = sampler(CASES[4]).sample_numpy(3, 64, 2, 1, stats)
    assert stats["unplaced"] == [10, 24] and int(unp.sum()) == 34, stats


def test_deterministic_and_draw_dependent():
    s = sampler(CASES[0])
    a, b = s.sample_numpy(5, 8, 3, 1), sampler(CASES[0]).sample_numpy(5, 8, 3, 1)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    other = s.sample_numpy(5, 8, 3, 2)[0]
    assert not np.any(np.all(other[:, :, :2] == a[0][:, :, :2], axis=(2, 3)))  # no route survives another draw
    assert not np.array_equal(RouteSampler(CASES[0][2], 3.0, 8.0, seed=42).sample_numpy(5, 8, 3, 1)[0], a[0])


def test_layout():
    wp, npts, unp = sampler(CASES[0]).sample_numpy(5, 8, 4, 1)
    assert wp.shape == (5, 8, 4, 3) and wp.dtype == np.float64
    assert npts.shape == (5, 8) and npts.dtype == np.int32 and np.all(npts == 2)
    assert unp.shape == (5,) and unp.dtype == np.int32
    assert np.array_equal(wp[:, :, 2], wp[:, :, 1]) and np.array_equal(wp[:, :, 3], wp[:, :, 1])
    w = sampler(CASES[0]).world(5, 8, 1, P=4)
    assert np.array_equal(w.waypoints, wp) and np.array_equal(w.n_points, npts) and w.buildings.shape == (0, 4)


def test_env_routes_do_not_depend_on_the_batch():
    """Env e draws from counter word e + env_offset: env_offset = 3, E = 2 is envs 3 and 4 of E = 5."""
    for case in (CASES[0], CASES[1]):
        N = case[1]
        whole = sampler(case).sample_numpy(5, N, 2, 1)
        part = sampler(case, env_offset=3).sample_numpy(2, N, 2, 1)
        for w, p in zip(whole, part):
            assert np.array_equal(w[3:5], p)
        assert np.array_equal(sampler(case).sample_numpy(2, N, 2, 1)[0], whole[0][:2])


@pytest.mark.parametrize("case", CASES)
def test_box_grid_and_separations(case):
    E, N, size, sep, length, _ = case
    s = sampler(case)
    wp, _, unp = s.sample_numpy(E, N, 2, 1)
    assert np.all(wp >= s.lo) and np.all(wp <= s.hi)
    assert np.array_equal(np.rint(wp * 100.0) / 100.0, wp)
    checked = 0
    for e in range(E):
        if unp[e]:
            continue
        for k in (0, 1):
            p = wp[e, :, k]
            d = p[:, None] - p[None]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert np.all(d2[~np.eye(N, dtype=bool)] >= sep * sep)
        d = wp[e, :, 1] - wp[e, :, 0]
        assert np.all((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] >= length * length)
        checked += 1
    if case[5] == 32:  # (32 rounds placed everybody: no env was skipped)
        assert checked == E


def test_c_abi_refuses_before_the_first_hip_call():
    """Every argument check of rvo3d_sample_routes / rvo3d_set_routes precedes the first HIP call: the refusals come
    back as RVO3D_ERR_INVALID (-1) with the argument's name on a machine without a GPU."""
    import ctypes as C
    from rvo3d_amd import _lib
    _lib.build_hip()
    L = _lib.lib()
    buf = (C.c_double * 8)()  # never dereferenced: the calls below are refused
    p = C.cast(buf, C.c_void_p)

    def call(cfg, E=2, N=8, P=2, wp=p, npts=p):
        return L.rvo3d_sample_routes(None if cfg is None else C.byref(cfg), E, N, P, 1, None, wp, npts, None, None)

    good = RouteSampler((20.0, 20.0, 8.0))
    for bad, word in ((dict(max_tries=0), b"max_tries"), (dict(max_tries=1025), b"max_tries"),
                      (dict(min_sep=-1.0), b"min_sep"), (dict(min_len=float("nan")), b"min_len")):
        cfg = good.config()
        for k, v in bad.items():
            setattr(cfg, k, v)
        assert call(cfg) == -1 and word in L.rvo3d_last_error(), bad
    for lo, hi in ((5.0, 5.0), (6.0, 5.0), (float("nan"), 5.0), (1.0, float("inf"))):
        cfg = good.config()
        cfg.lo[1], cfg.hi[1] = lo, hi
        assert call(cfg) == -1 and b"lo / hi" in L.rvo3d_last_error()
    cfg = good.config()
    assert call(cfg, N=513) == -1 and b"num_drones" in L.rvo3d_last_error()
    assert call(cfg, N=0) == -1 and call(cfg, E=0) == -1
    assert call(cfg, P=1) == -1 and b"max_points" in L.rvo3d_last_error()
    assert call(cfg, wp=None) == -1 and b"waypoints" in L.rvo3d_last_error()
    assert call(cfg, npts=None) == -1 and b"n_points" in L.rvo3d_last_error()
    assert call(None) == -1 and b"cfg" in L.rvo3d_last_error()
    assert L.rvo3d_set_routes(None, None, p, p, None) == -1 and b"handle" in L.rvo3d_last_error()
    assert L.rvo3d_get_routes(None, p, p, None) == -1


def test_argument_checks():
    with pytest.raises(ValueError):
        RouteSampler((2.0, 20.0, 8.0), margin=1.0)  # lo == hi
    with pytest.raises(ValueError):
        RouteSampler((20.0, 20.0, 8.0), max_tries=0)
    with pytest.raises(ValueError):
        RouteSampler((20.0, 20.0, 8.0), min_sep=-1.0)
    with pytest.raises(ValueError):
        RouteSampler((20.0, 20.0, 8.0)).sample_numpy(1, 513, 2, 0)
