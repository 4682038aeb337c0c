"""The fused step after its memory round trips were shortened (csrc/rvo3d_step.hpp: one load batch in phase 0, the
map's bounds and T04 read once, the old row count clamped where it is filed): the places where the reading order
changed, each against the CPU oracle with the parity tests' own comparison (test_gpu_parity.Tally: flags and counts
bit-exact, observations and rewards f32-exact, knife-edge accounting) or bit for bit against a full-write step.

  * map bounds: drones put just outside each of the six faces, exactly on each upper bound (`>` is strict: inside)
    and with a NaN coordinate - the test is now six compares joined with `|` on bounds read ahead of the stores;
  * old row counts: prev_vo_count rows of nm + 1, INT32_MAX and -1 are clamped after the load batch, not in it;
  * action paths: float32 / float64 absolute actions with and without re-quantisation, and the policy increment,
    are loaded into variables of their own.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as orc
from golden_util import eq_nan
from rvo3d_amd import BatchedDroneEnv, World, _lib, synthetic_actions, synthetic_world
from test_gpu_parity import Tally, close, resync_from_oracle

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1


def _oracle(world, nm=10):
    return orc.OracleEnv(world.waypoints, world.n_points, world.map_size, world.buildings, nm=nm, threads=8)


def step_both(run, env, ref, a_ref, autoreset, tl, t, strict=None):
    """One step on both sides - run() steps the device and returns its six outputs - compared as
    test_gpu_parity.run_vs_oracle compares it.  `strict` [E, N]: samples that are compared without the knife-edge
    exemption (their margin is zero by construction)."""
    obs, cnt, rew, done, info, fin = run()
    if autoreset:
        ro, rcnt, rr, rd, ri, rf, rm = ref.step_autoreset(a_ref)
    else:
        ro, rcnt, rr, rd, ri, rf = ref.step(a_ref)
        rm = None
    mg = ref.margin().copy()
    if strict is not None:
        mg[strict] = np.inf
    tl.begin(mg)
    if autoreset:
        tl.check(f"reset_mask t={t}", env.reset_mask.cpu().numpy() == rm)
    o, r = obs.cpu().numpy(), rew.cpu().numpy()
    tl.check(f"done t={t}", done.cpu().numpy() == rd)
    tl.check(f"info t={t}", info.cpu().numpy() == ri)
    tl.check(f"finish t={t}", fin.cpu().numpy() == rf)
    tl.check(f"vo_count t={t}", cnt.cpu().numpy() == rcnt)
    tl.check(f"obs t={t}", close(o, ro))
    tl.check(f"reward t={t}", close(r, rr))
    tl.check(f"obs f32-exact t={t}", eq_nan(o, ro.astype(np.float32)))
    tl.check(f"reward f32-exact t={t}", eq_nan(r, rr.astype(np.float32)))
    tl.end()
    return rd, rm


def assert_state_equal(env, ref, tl):
    assert not tl.dropped.any()
    s, rs = env.get_state(), ref.get_state()
    for k in ("wp_idx", "arrive", "dest"):
        assert np.array_equal(s[k].cpu().numpy(), rs[k]), k
    for k in ("pos", "vel", "yaw", "pitch", "real_len", "max_dev", "extra_len"):
        np.testing.assert_allclose(s[k].cpu().numpy(), rs[k], rtol=1e-9, atol=1e-9, err_msg=k)


# ---- map bounds ---------------------------------------------------------------------------------------------------
MAP = (30.0, 30.0, 10.0)
UP = lambda x: float(np.nextafter(x, np.inf))
TINY = -1e-12
# ten drones per env, at rest and far from each other: the post-move position is the one set here
OUTSIDE = [(TINY, 5.0, 5.0), (UP(MAP[0]), 8.0, 5.0), (5.0, TINY, 5.0), (8.0, UP(MAP[1]), 5.0),
           (12.0, 5.0, TINY), (12.0, 8.0, UP(MAP[2]))]
ON_BOUND = [(MAP[0], 12.0, 5.0), (15.0, MAP[1], 5.0), (15.0, 12.0, MAP[2])]
WITH_NAN = [(float("nan"), 20.0, 5.0)]
PLACED = OUTSIDE + ON_BOUND + WITH_NAN


def _place(E, N, t, state):
    """Put the ten drones into every env, at drone indices that move with the env and the step (every lane
    position of a wave is met, the partial last workgroup of 16 x 5 included).  Returns the index arrays."""
    pos, vel = state["pos"].copy(), state["vel"].copy()
    idx = np.empty((E, len(PLACED)), np.int64)
    for e in range(E):
        idx[e] = (3 * e + 5 * t + np.arange(len(PLACED)) * (N // len(PLACED))) % N
        assert len(set(idx[e])) == len(PLACED)
        pos[e, idx[e]] = np.array(PLACED)
        vel[e, idx[e]] = 0.0
    return pos, vel, idx


@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("N,E", [(16, 5), (64, 2), (128, 2)])
def test_map_bounds(N, E, autoreset):
    world = synthetic_world(E, N, MAP, seed=31)
    env, ref = BatchedDroneEnv(world), _oracle(world)
    env.observe(); ref.observe()
    tl = Tally(f"round_trips/map_{N}x{E}_{int(autoreset)}", E)
    rows = np.arange(E)[:, None]
    for t in range(2):
        env.reset(); ref.reset()  # (the ten of the last step are not left standing where the next ten go)
        pos, vel, idx = _place(E, N, t, ref.get_state())
        env.set_state(pos=pos, vel=vel); ref.set_state(pos=pos, vel=vel)
        a = synthetic_actions(E, N, t, seed=17)
        a[rows, idx] = 0.0  # speed 0 + acceleration 0: nobody of the ten moves
        strict = np.zeros((E, N), bool)
        strict[rows, idx] = True
        ad = torch.from_numpy(a).cuda()
        rd, rm = step_both(lambda: env.step(ad, autoreset=autoreset), env, ref, a, autoreset, tl, t, strict)
        # the oracle itself says the ten are what they were placed as (nobody else came near them)
        no = len(OUTSIDE)
        assert (rd[rows, idx[:, :no]] == 1).all()
        assert (rd[rows, idx[:, no:]] == 0).all(), "a drone on an upper bound or with a NaN coordinate collided"
        if autoreset:
            assert (rm[rows, idx[:, :no]] == 1).all()
        resync_from_oracle(env, ref, tl)
        assert_state_equal(env, ref, tl)
    assert env.error_flags() & 1  # the NaN coordinate reached an observation
    assert ref.nan_count > 0
    env.close()
    print(tl.finish())


# ---- old row counts -----------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _grid_world(E, N, pitch=4.0):
    """A grid of starts in one plane, `pitch` apart (nobody's velocity obstacle reaches a neighbour), all flying +x."""
    side = int(np.ceil(np.sqrt(N)))
    g = np.array([(3.0 + pitch * (k % side), 3.0 + pitch * (k // side), 5.0) for k in range(N)])
    wp = np.empty((E, N, 2, 3))
    for e in range(E):
        wp[e, :, 0] = np.roll(g, 7 * e, axis=0)
        wp[e, :, 1] = wp[e, :, 0] + np.array([40.0, 0.0, 0.0])
    L = 3.0 + pitch * side
    return World(wp, np.full((E, N), 2, np.int32), np.array([L + 45.0, L + 3.0, 10.0]))


def _head_on(state):
    """Every odd drone 2 m in front of its even neighbour (and a little beside it), the two flying at each other at
    0.5 m per step: with an acceleration of 0.2 the step ends 0.6 m apart - no collision - and the even drone keeps
    a VO row (decision margin 1.5e-4 in the oracle); one step later they have passed each other and the rows are
    gone (checked on the oracle: nobody resets in either step)."""
    pos, vel, yaw = state["pos"].clone(), state["vel"].clone(), state["yaw"].clone()
    N = pos.shape[1]
    for k in range(0, N - 1, 2):
        pos[:, k + 1] = pos[:, k] + torch.tensor([2.0, 0.13, 0.07], dtype=pos.dtype, device=pos.device)
        vel[:, k] = torch.tensor([0.5, 0.0, 0.0], dtype=pos.dtype, device=pos.device)
        vel[:, k + 1] = -vel[:, k]
        yaw[:, k] = 0.0; yaw[:, k + 1] = 180.0
    return dict(pos=pos, vel=vel, yaw=yaw)


@pytest.mark.parametrize("kind", ["head_on", "crowded"])
@pytest.mark.parametrize("N,E", [(64, 3), (16, 5), (128, 2)])
def test_old_counts_out_of_range(N, E, kind):
    """rvo3d_step_ex with prev_vo_count rows of nm + 1, INT32_MAX and -1 and a NaN sentinel in those rows' VO region:
    such a row promises nothing, every byte of it is written; the other rows carry their true old counts.
    "crowded" is the world of tests/test_gpu_obs_reuse.py; at these sizes the oracle keeps at most two VO rows in it
    over the six steps (an env that resets a drone is observed with action 0), so "head_on" is the world that keeps
    them: half the rows get a VO row in steps 0 and 2 and lose it in steps 1 and 3."""
    nm = 10
    if kind == "crowded":
        world = synthetic_world(E, N, (9.0, 9.0, 4.0), n_points=3, seed=7, min_sep=0.5)
    else:
        world = _grid_world(E, N)
    fast = BatchedDroneEnv(world, neighbors_num=nm)
    full = BatchedDroneEnv(world, neighbors_num=nm, reuse_obs=False)
    fast.observe(); full.observe()
    bad_values = [nm + 1, INT32_MAX, -1]
    rng = np.random.default_rng(3)
    old_rows = new_rows = bad_new_rows = 0
    for t in range(4 if kind == "head_on" else 6):
        if kind == "head_on":
            if t % 2 == 0:
                st = _head_on(full.get_state())
                fast.set_state(**st); full.set_state(**st)
            a = torch.zeros((E, N, 3), dtype=torch.float64, device="cuda")
            a[..., 0] = 0.2
        else:
            a = torch.from_numpy(synthetic_actions(E, N, t, seed=11)).cuda()
        prev = fast.vo_count.clone()
        old_rows += int((prev > 0).sum())
        # the first and the last row, and a tenth of the others
        rows = np.unique(np.concatenate([[0, E * N - 1], rng.choice(E * N, E * N // 10, replace=False)]))
        vals = torch.tensor([bad_values[i % 3] for i in range(len(rows))], dtype=torch.int32).cuda()
        ridx = torch.from_numpy(rows).cuda()
        prev.view(-1)[ridx] = vals
        fast.obs.view(E * N, -1)[ridx, 12:] = float("nan")  # the sentinel
        args = _lib.StepArgs()
        args.actions = a.data_ptr(); args.action_dtype = _lib.RVO3D_F64; args.policy = 0; args.autoreset = 1
        args.obs = fast.obs.data_ptr(); args.vo_count = fast.vo_count.data_ptr()
        args.reward = fast.reward.data_ptr(); args.done = fast.done.data_ptr()
        args.info = fast.info.data_ptr(); args.finish = fast.finish.data_ptr()
        args.reset_mask = fast.reset_mask.data_ptr(); args.prev_vo_count = prev.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().rvo3d_step_ex(fast._h, C.byref(args), stream), "rvo3d_step_ex")
        torch.cuda.synchronize()
        full.obs.fill_(float("nan")); full.vo_count.fill_(-7)
        full.step(a, autoreset=True)
        assert not torch.isnan(fast.obs).any(), f"step {t}: a sentinel survived"
        assert torch.equal(_bits(fast.obs), _bits(full.obs)), f"step {t}"
        assert torch.equal(fast.vo_count, full.vo_count), f"step {t}"
        new_rows += int((fast.vo_count > 0).sum())
        bad_new_rows += int((fast.vo_count.view(-1)[ridx] > 0).sum())
    if kind == "head_on":  # rows kept before, rows kept now, rows kept in rows whose old count was out of range
        assert old_rows > 0 and new_rows > 0 and bad_new_rows > 0, (old_rows, new_rows, bad_new_rows)
    fast.close(); full.close()


# ---- action paths -------------------------------------------------------------------------------------------------
ACCELER = 0.5


def _quantise(a, dec):
    s = 10.0 ** dec
    return np.rint(a * s) / s  # the kernel's own sequence (act_scale), in float64


@pytest.mark.parametrize("kind,dec", [("f32", 0), ("f32", 2), ("f64", 0), ("f64", 2), ("policy", -1)])
def test_action_paths(kind, dec):
    """32 drones x 3 envs (two envs per wave, a partial last workgroup), fused auto-reset steps.  The device gets
    the raw samples - not multiples of 10^-dec - in the type of the case; the oracle gets what the step makes of
    them: the re-quantised float64 action, or the trainer's glue (multi_ppo.py:196-205) for a policy increment."""
    E, N, T = 3, 32, 6
    world = synthetic_world(E, N, (12.0, 12.0, 5.0), seed=5, min_sep=0.5)
    env = BatchedDroneEnv(world, action_decimals=dec, acceler=ACCELER)
    ref = _oracle(world)
    env.observe(); ref.observe()
    tl = Tally(f"round_trips/action_{kind}_{dec}", E)
    resets = 0
    for t in range(T):
        rng = np.random.Generator(np.random.Philox(key=99, counter=[0, 0, 0, t]))
        raw = rng.uniform(-1, 1, (E, N, 3)) * np.array([1.0, 0.3, 0.15])
        if dec == 0:
            # whole-number accelerations of 0 and 1 only: with -1 among them `speed + acc` would cancel to libm
            # noise in one drone-step of eight (the oracle's knife edge at drone.py:452; 73 of 576 samples here,
            # against the 1 % the parity accounting allows its inputs)
            raw[..., 0] = 0.5 + 0.9 * raw[..., 0]
        if kind == "policy":
            inc = torch.from_numpy(raw.astype(np.float32)).cuda()
            r = np.rint(raw.astype(np.float32) * np.float32(100.0)) / np.float32(100.0)
            x = (np.float32(ACCELER) * r).astype(np.float64) + ref.get_state()["vel"]
            a_ref = np.rint(x * 100.0) / 100.0
            run = lambda: env.step_policy(inc, autoreset=True)
        else:
            dev = raw.astype(np.float32) if kind == "f32" else raw
            a_ref = _quantise(dev.astype(np.float64), dec)
            a_env = torch.from_numpy(dev).cuda()
            run = lambda: env.step(a_env, autoreset=True)
        rd, rm = step_both(run, env, ref, a_ref, True, tl, t)
        resets += int(rm.sum())
        resync_from_oracle(env, ref, tl)
    assert resets > 0
    assert_state_equal(env, ref, tl)
    env.close()
    print(tl.finish(resets=resets))
