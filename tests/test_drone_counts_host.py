"""Per-env drone counts, the parts that need no GPU: the host set-up (csrc/rvo3d_host_setup.hpp: check_drone_counts,
pick_counted_kernel, counted_geometry - C++, checked by the stand-alone program tests/host/drone_counts_check.hip, built
here with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and run as a child process), the worlds
(World.drone_counts, select, with_max_points, stack_worlds, sharding) and the trainer's data path (RolloutBuffer.get() with
a live mask, multi_ppo.update on data with ghost rows)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from rvo3d_amd import _lib, sharding
from rvo3d_amd.policy import mlp_ac, multi_ppo
from rvo3d_amd.policy.multi_ppo import RolloutBuffer
from rvo3d_amd.worlds import stack_worlds, synthetic_world

CSRC = os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "drone_counts_check.hip")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-O1",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
MAP = (30.0, 30.0, 12.0)


def test_drone_counts_host_setup_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "drone_counts_check")
    subprocess.check_call([hipcc] + FLAGS + ["-I", CSRC, "-o", exe, SRC])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout)
    print(res.stderr)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "drone counts ok" in res.stdout


def test_the_library_declares_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "rvo3d.h")).read()
    for s in ("rvo3d_set_drone_counts", "rvo3d_drone_counts", "rvo3d_rollout_account_n"):
        assert f"int {s}(" in hdr and s in _lib.SYMBOLS and hasattr(_lib.lib(), s)


def test_world_carries_drone_counts():
    w = synthetic_world(5, 6, MAP, n_points=3, seed=3)
    assert w.drone_counts is None and w.env_drones(2) == 6
    c = np.array([6, 1, 4, 2, 6])
    k = w.with_drone_counts(c)
    assert k.drone_counts.dtype == np.int32 and k.drone_counts.tolist() == c.tolist()
    assert [k.env_drones(e) for e in range(5)] == c.tolist() and k.shape == w.shape
    assert k.waypoints is w.waypoints and w.drone_counts is None          # the routes are shared, the original untouched
    c[0] = 3
    assert k.drone_counts[0] == 6                                          # a copy
    for bad in ([0, 1, 1, 1, 1], [7, 1, 1, 1, 1], [1, 1, 1], [[1, 1, 1, 1, 1]]):
        with pytest.raises(ValueError):
            w.with_drone_counts(bad)
    assert k.with_drone_counts(None).drone_counts is None
    # select: indices, a slice and a mask
    assert k.select([3, 0]).drone_counts.tolist() == [2, 6]
    assert k.select(slice(1, 4)).drone_counts.tolist() == [1, 4, 2]
    assert k.select(np.arange(5) % 2 == 0).drone_counts.tolist() == [6, 4, 6]
    assert w.select([1]).drone_counts is None
    p = k.with_max_points(5)
    assert p.drone_counts.tolist() == k.drone_counts.tolist() and p.shape == (5, 6, 5)


def test_stack_worlds_pads_fleets_of_different_sizes():
    a, b, c = synthetic_world(2, 2, MAP, seed=1), synthetic_world(1, 4, MAP, n_points=3, seed=2), synthetic_world(2, 8, MAP, seed=3)
    with pytest.raises(ValueError):
        stack_worlds([a, b, c])                       # as before: different drone counts need the opt-in
    s = stack_worlds([a, b, c], pad_drones=True)
    assert s.shape == (5, 8, 3) and s.drone_counts.tolist() == [2, 2, 4, 8, 8] and s.drone_counts.dtype == np.int32
    # the live rows are the worlds' own routes (padded with their destination) ...
    assert np.array_equal(s.waypoints[0:2, :2, :2], a.waypoints) and np.array_equal(s.waypoints[0:2, :2, 2], a.waypoints[:, :, 1])
    assert np.array_equal(s.waypoints[2, :4], b.waypoints[0])
    assert np.array_equal(s.waypoints[3:], np.concatenate([c.waypoints, c.waypoints[:, :, 1:2]], 2))
    assert np.array_equal(s.n_points[2, :4], b.n_points[0]) and np.array_equal(s.n_points[0:2, :2], a.n_points)
    # ... the ghost rows a copy of the env's drone 0 route, cut to its first leg
    for e, n in enumerate(s.drone_counts):
        assert np.all(s.n_points[e, n:] == 2)
        assert np.array_equal(s.waypoints[e, n:, :2], np.repeat(s.waypoints[e, :1, :2], 8 - n, 0))
        assert np.array_equal(s.waypoints[e, n:, 2], s.waypoints[e, n:, 1])
    # equal counts: nothing to say; the map-size rule stays; counts of the inputs are kept
    assert stack_worlds([a, a], pad_drones=True).drone_counts is None and stack_worlds([a, a]).drone_counts is None
    with pytest.raises(ValueError):
        stack_worlds([a, synthetic_world(1, 4, (40.0, 30.0, 12.0), seed=5)], pad_drones=True)
    k = stack_worlds([c.with_drone_counts([3, 8]), b], pad_drones=True)
    assert k.drone_counts.tolist() == [3, 8, 4]
    assert stack_worlds([c.with_drone_counts([3, 8]), c]).drone_counts.tolist() == [3, 8, 8, 8]


def test_sharding_cuts_the_counts_with_the_envs():
    w = synthetic_world(7, 4, MAP, seed=4, nb=3, per_env_buildings=True).with_drone_counts([4, 1, 2, 3, 4, 2, 1])
    got = []
    for r in range(3):
        s = sharding.shard_world(w, r, 3)
        lo, hi = sharding.shard_env_range(7, r, 3)
        assert s.shape[0] == hi - lo and np.array_equal(s.waypoints, w.waypoints[lo:hi])
        assert np.array_equal(s.buildings, w.buildings[lo:hi])
        got += s.drone_counts.tolist()
    assert got == w.drone_counts.tolist()


def _filled(T, E, N, W, live, seed):
    g = torch.Generator().manual_seed(seed)
    buf = RolloutBuffer(T, E, N, W, 3, "cpu", 0.99, 0.97, live=live)
    for t in range(T):
        buf.store(torch.randn(E, N, W, generator=g), torch.zeros(E, N, dtype=torch.int32), torch.randn(E, N, 3, generator=g),
                  torch.randn(E, N, generator=g), torch.randn(E, N, generator=g), torch.randn(E, N, generator=g))
        buf.finish_path(torch.rand(E, generator=g) < 0.3)
    return buf


def test_rollout_buffer_get_hands_out_the_live_rows():
    T, E, N, W = 5, 4, 3, 21
    counts = torch.tensor([3, 1, 2, 3])
    live = torch.arange(N)[None, :] < counts[:, None]
    full, part = _filled(T, E, N, W, None, 7).get(), _filled(T, E, N, W, live, 7).get()
    assert "live" not in full and full["obs"].shape[0] == T * E * N and full["shape"] == (T, E, N)
    rows = live.unsqueeze(0).expand(T, E, N).reshape(-1)
    assert part["shape"] == (T, E, N) and torch.equal(part["live"], live)
    for k in ("obs", "cnt", "act", "ret", "adv", "logp"):
        assert part[k].shape[0] == T * int(counts.sum()), k
        assert torch.equal(part[k], full[k][rows]), k            # t, e, n order, the ghost rows removed, nothing else changed


class _Env:
    """What multi_ppo reads of an env at construction."""
    W, device = 21, torch.device("cpu")

    def __init__(self, E, N, counts=None):
        self.E, self.N = E, N
        self.drone_counts = None if counts is None else torch.as_tensor(counts, dtype=torch.int32)
        self.live = torch.ones(E, N, dtype=torch.bool) if counts is None else \
            torch.arange(N)[None, :] < self.drone_counts[:, None]


def _trainer(env, **kw):
    torch.manual_seed(0)
    ac = mlp_ac(21, hidden_sizes=(16, 16))
    return multi_ppo(env, ac, steps_per_epoch=5, train_pi_iters=2, train_v_iters=2, target_kl=1e9, use_gpu=False, seed=5,
                     **kw), ac


def _params(ac):
    return torch.cat([p.detach().reshape(-1) for p in ac.parameters()])


@pytest.mark.parametrize("reference_order", [False, True])
def test_update_on_ghost_rows_equals_the_update_without_them(reference_order):
    """2 + 2 iterations on a buffer with ghost rows leave the parameters bit-equal to an update on the same data with the
    ghost rows deleted by hand; with no counts the update is what it was."""
    T, E, N, W = 5, 4, 3, 21
    counts = [3, 1, 2, 3]
    env = _Env(E, N, counts)
    tr, ac = _trainer(env, reference_order=reference_order)
    assert tr.robot_num == 3 and torch.equal(tr.buf.live, env.live)
    full = _filled(T, E, N, W, None, 11).get()
    tr.buf = _filled(T, E, N, W, env.live, 11)
    st = tr.update(tr.buf.get())

    tr2, ac2 = _trainer(_Env(E, N), reference_order=reference_order)
    rows = env.live.unsqueeze(0).expand(T, E, N).reshape(-1)
    by_hand = {k: v[rows] for k, v in full.items() if k != "shape"}
    if reference_order:
        # agent r: drone r of the envs that have one, all steps - the reference's own signature, a dict per agent
        drone = torch.arange(N).expand(T, E, N).reshape(-1)[rows]
        st2 = tr2.update([{k: v[drone == r] for k, v in by_hand.items()} for r in range(3)])
        assert st["order"] == st2["order"] and st["pi_steps"] == st2["pi_steps"]
        assert [int((drone == r).sum()) for r in range(3)] == [T * 4, T * 3, T * 2]
    else:
        st2 = tr2.update(dict(by_hand, shape=(T, E, N)))          # (ragged: the pooled update never looks at the shape)
        assert st["pi_steps"] == st2["pi_steps"] == 2
    assert torch.equal(_params(ac), _params(ac2))
    assert st["kl"] == st2["kl"] and st["loss_v"] == st2["loss_v"]

    # no counts: the data has no live mask and the update is the one of a trainer that never heard of counts
    tr3, ac3 = _trainer(_Env(E, N), reference_order=reference_order)
    tr4, ac4 = _trainer(_Env(E, N), reference_order=reference_order)
    assert tr3.live is None and tr3.robot_num == N
    tr3.buf = _filled(T, E, N, W, None, 11)
    data = tr3.buf.get()
    assert set(data) == {"obs", "cnt", "act", "ret", "adv", "logp", "shape"}
    tr3.update(data)
    tr4.update({k: (v.clone() if torch.is_tensor(v) else v) for k, v in full.items()})
    assert torch.equal(_params(ac3), _params(ac4)) and not torch.equal(_params(ac3), _params(ac))


def test_truncated_world_keeps_its_building_counts():
    """The yardstick helper of tests/test_gpu_drone_counts.py on a world of per-env sets: the listed envs with their
    first c drones, their own sets and their own set sizes; the per-env scene has an empty and a full set."""
    from test_gpu_drone_counts import BLD_SCENES, building_scene, truncated
    world, counts = building_scene(21, 8, True)
    nb = world.buildings.shape[1]
    assert counts.tolist() == [21, 1, 3, 5, 2, 8, 7, 21] and world.building_counts[0] == nb and world.building_counts[2] == 0
    envs = np.array([2, 5, 7])
    w = truncated(world, envs, 3)
    assert w.shape == (3, 3, 2) and np.array_equal(w.waypoints, world.waypoints[envs, :3])
    assert np.array_equal(w.buildings, world.buildings[envs]) and np.array_equal(w.building_counts, world.building_counts[envs])
    shared, _ = building_scene(21, 8, False)
    w = truncated(shared, envs, 3)
    assert w.building_counts is None and np.array_equal(w.buildings, shared.buildings) and len(shared.buildings) == nb
    assert len(BLD_SCENES) == 6
