"""CPU-side checks of the biGRU tiles feature: crossing_world's geometry, the new C-ABI symbols (exported, declared,
with the ctypes signatures of _lib), their size queries, and argument checks that fail before anything touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from rvo3d_amd import _lib, crossing_world

NEW = ("rvo3d_policy_rnn_tiles_blob_bytes", "rvo3d_policy_rnn_tiles_pack", "rvo3d_policy_rnn_tiles_work_bytes",
       "rvo3d_policy_rnn_tiles")


@pytest.fixture(scope="module")
def L():
    _lib.build_hip()
    return _lib.lib()


def test_crossing_world_geometry():
    E, N, ms = 6, 64, (30.0, 30.0, 10.0)
    w = crossing_world(E, N, ms, seed=3)
    assert w.waypoints.shape == (E, N, 2, 3) and (w.n_points == 2).all() and w.buildings.shape == (0, 4)
    c = np.array(ms) / 2
    start, dest = w.waypoints[:, :, 0], w.waypoints[:, :, 1]
    np.testing.assert_allclose(start + dest, np.broadcast_to(2 * c, start.shape), atol=1e-9)           # antipodal through the centre
    np.testing.assert_array_equal(np.round(start, 2), start)
    for p in (start, dest):                                                # inside the map, 1 m margin
        assert (p >= 1.0).all() and (p <= np.array(ms) - 1.0).all()
    for e in range(E):                                                     # starts min_sep apart
        d = np.linalg.norm(start[e][:, None] - start[e][None], axis=-1) + np.eye(N) * 99
        assert d.min() >= 1.0
    # a ring: every start at radius 12 +- 0.5 from the centre's vertical axis, altitude c_z +- 1
    rr = np.linalg.norm(start[..., :2] - c[:2], axis=-1)
    assert (np.abs(rr - 12.0) <= 0.5 + 0.01).all() and (np.abs(start[..., 2] - c[2]) <= 1.0 + 0.01).all()
    # everyone heads at the centre: the swap scene
    head = dest - start
    to_c = c - start
    cos = (head * to_c).sum(-1) / np.linalg.norm(head, axis=-1) / np.linalg.norm(to_c, axis=-1)
    assert (cos > 0.999).all()
    w2 = crossing_world(E, N, ms, seed=3)
    assert np.array_equal(w.waypoints, w2.waypoints)                       # deterministic per seed
    assert not np.array_equal(w.waypoints, crossing_world(E, N, ms, seed=4).waypoints)
    with pytest.raises(ValueError):
        crossing_world(1, 8, (10.0, 10.0, 4.0), radius=6.0)                 # does not fit
    with pytest.raises(ValueError):
        crossing_world(1, 200, (10.0, 10.0, 4.0), radius=3.0)               # no room for 200 starts 1 m apart


def test_new_symbols_declared_and_exported(L):
    hdr = open(os.path.join(ROOT, "include", "rvo3d.h")).read()
    declared = set(re.findall(r"\b(rvo3d_[a-z_0-9]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s)


def test_size_queries(L):
    b = L.rvo3d_policy_rnn_tiles_blob_bytes
    sizes = {(h, bi): b(h, 9, 12, bi) for h in (64, 256) for bi in (0, 1)}
    assert all(v > 0 and v % 16 == 0 for v in sizes.values())
    assert sizes[(256, 1)] > sizes[(256, 0)] > sizes[(64, 1)] > sizes[(64, 0)]
    assert sizes[(256, 1)] - sizes[(256, 0)] > 384 * 1024                   # a second W_hh of 768 x 256 bf16
    for bad in ((128, 9, 12, 1), (0, 9, 12, 1), (256, 8, 12, 1), (256, 9, 0, 1), (256, 9, 17, 0)):
        assert b(*bad) == -1
    assert L.rvo3d_policy_rnn_tiles_work_bytes(1000, 10) == 4 * (32 + 10 * 1000)
    assert L.rvo3d_policy_rnn_tiles_work_bytes(1000, 13) == -1 and L.rvo3d_policy_rnn_tiles_work_bytes(0, 4) == -1


def _fake(n):
    return C.c_void_p(4096 * n)   # (never dereferenced: every call below fails its argument checks first)


def test_bad_arguments_fail_before_any_launch(L):
    nb = L.rvo3d_policy_rnn_tiles_blob_bytes(256, 9, 12, 1)

    def call(**kw):
        a = dict(blob=_fake(1), blob_bytes=nb, hidden=256, in_dim=9, state_dim=12, bidir=1, obs=_fake(2), obs_ld=102,
                 cnt=_fake(3), lst=_fake(4), count=_fake(5), done=_fake(6), work=_fake(7), max_rows=1000, slots=10,
                 tanh=1, log_std=_fake(8), std=1.0, seed=7, step=0, act=_fake(9), logp=_fake(10), val=_fake(11),
                 mu=None, stream=None)
        a.update(kw)
        return L.rvo3d_policy_rnn_tiles(*a.values())

    for kw in (dict(hidden=128), dict(hidden=64), dict(in_dim=8), dict(state_dim=17), dict(slots=0), dict(slots=13),
               dict(bidir=0), dict(blob_bytes=nb - 16), dict(obs=None), dict(cnt=None), dict(lst=None),
               dict(count=None), dict(done=None), dict(work=None), dict(act=None), dict(logp=None), dict(val=None),
               dict(log_std=None), dict(blob=None), dict(obs_ld=101), dict(max_rows=0), dict(blob=C.c_void_p(4096 + 8))):
        assert call(**kw) == -1, kw
        assert L.rvo3d_last_error()
    assert call(hidden=64) == -1 and b"another" in L.rvo3d_last_error()
    # pack: null pointers, the shape, the blob size
    w = [_fake(20 + i) for i in range(10)]
    net = _lib.RnnPolicy(*w, 256, 9, 12, 0, 1e-5, 0, _lib.MlpWeights(*[_fake(40 + i) for i in range(6)]),
                         _lib.MlpWeights(*[_fake(50 + i) for i in range(6)]))
    pk = L.rvo3d_policy_rnn_tiles_pack
    assert pk(None, _fake(1), nb, None) == -1
    assert pk(C.byref(net), None, nb, None) == -1
    assert pk(C.byref(net), _fake(1), nb - 16, None) == -1
    assert pk(C.byref(net), _fake(1), L.rvo3d_policy_rnn_tiles_blob_bytes(256, 9, 12, 0), None) == -1  # packed for GRU
    for field, v in (("hidden", 100), ("in_dim", 10), ("state_dim", 20)):
        bad = _lib.RnnPolicy.from_buffer_copy(net)
        setattr(bad, field, v)
        assert pk(C.byref(bad), _fake(1), nb, None) == -1
    bad = _lib.RnnPolicy.from_buffer_copy(net)
    bad.w_hh_r = None                                                     # half a reverse direction
    assert pk(C.byref(bad), _fake(1), nb, None) == -1
    bad = _lib.RnnPolicy.from_buffer_copy(net)
    bad.pi.w2 = None
    assert pk(C.byref(bad), _fake(1), nb, None) == -1
