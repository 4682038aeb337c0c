"""Observation reuse (rvo3d_step_args.prev_vo_count): a step into the env's own obs / vo_count, while the
pair is still what the library last wrote, leaves out the stores of zeros the buffer already holds.  The
bytes it returns must be exactly those of a step that writes every byte."""
import ctypes as C

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, _lib, synthetic_actions, synthetic_world

pytestmark = pytest.mark.gpu

# crowded worlds: many VO rows that come and go, collisions and arrivals (auto-resets) every step.
# (E, N): one-wave workgroups of 1 / 4 envs, a padded one-wave kernel (40 of 64 lanes), two-wave workgroups,
# and E not a multiple of the envs per workgroup (a partial last workgroup: the row-pair writer)
SHAPES = [(64, 64), (33, 16), (24, 40), (6, 128)]
MAP = (9.0, 9.0, 4.0)


def _pair(E, N, seed=7, **kw):
    w = synthetic_world(E, N, MAP, n_points=3, seed=seed, min_sep=0.5)
    fast = BatchedDroneEnv(w, neighbors_num=10, **kw)
    full = BatchedDroneEnv(w, neighbors_num=10, reuse_obs=False, **kw)
    return fast, full


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


def _step_full(full, a):
    """The reference: fresh NaN-filled outputs every step (nothing of the last step survives)."""
    full.obs.fill_(float("nan"))
    full.vo_count.fill_(-7)
    return full.step(a, autoreset=True)


@pytest.mark.parametrize("E,N", SHAPES)
def test_reuse_bit_identical_to_full_writes(E, N):
    fast, full = _pair(E, N)
    fast.observe(); full.observe()
    seen_cnt, seen_reset, falls = 0, 0, 0
    prev = None
    for t in range(80):
        a = torch.from_numpy(synthetic_actions(E, N, t, seed=11)).cuda()
        assert fast._obs_ver == fast._own_versions()  # the fast path is taken
        of = fast.step(a, autoreset=True)
        oo = _step_full(full, a)
        _same(of, oo)
        assert torch.equal(fast.reset_mask, full.reset_mask)
        cnt = of[1].clone()
        seen_cnt += int((cnt > 0).sum())
        seen_reset += int(fast.reset_mask.sum())
        if prev is not None:
            falls += int((cnt < prev).sum())
        prev = cnt
    # the world exercised what the reuse depends on: kept rows that appear and disappear, resets
    assert seen_cnt > 0 and falls > 0 and seen_reset > 0
    fast.close(); full.close()


def test_reuse_step_policy_own_buffers():
    E, N = 64, 64
    fast, full = _pair(E, N)
    fast.observe(); full.observe()
    for t in range(64):
        g = torch.Generator().manual_seed(t)
        a = (torch.rand((E, N, 3), generator=g) * 2 - 1).cuda()
        of = fast.step_policy(a, autoreset=True)
        full.obs.fill_(float("nan")); full.vo_count.fill_(-7)
        oo = full.step_policy(a, autoreset=True)
        _same(of, oo)
    fast.close(); full.close()


def test_inplace_mutation_falls_back_to_full_writes():
    E, N = 64, 64
    fast, full = _pair(E, N)
    fast.observe(); full.observe()
    for t in range(24):
        a = torch.from_numpy(synthetic_actions(E, N, t, seed=3)).cuda()
        if t % 3 == 1:
            v = fast.obs[5:40]           # a view: shares the version counter
            v[:, :, 30:] = 1.5           # slice assignment
        elif t % 3 == 2:
            fast.vo_count.add_(1)        # counts that promise more kept rows than there are
            fast.obs.add_(0.25)
        _same(fast.step(a, autoreset=True), _step_full(full, a))
    fast.close(); full.close()


def _nan_left_after_step(env, a):
    """NaN written past torch's version counter (.data): a step that trusts the pair leaves some of it."""
    env.obs.data.fill_(float("nan"))
    env.step(a, autoreset=True)
    return bool(torch.isnan(env.obs).any())


def test_opt_out_and_invalidate_force_full_writes():
    E, N = 64, 64
    w = synthetic_world(E, N, (50.0, 50.0, 10.0))
    a = torch.from_numpy(synthetic_actions(E, N, 0)).cuda()
    env = BatchedDroneEnv(w, neighbors_num=10)
    env.observe()
    env.step(a, autoreset=True)
    # the fast path is live in env.step: stores of zeros are really left out
    assert _nan_left_after_step(env, a)
    env.obs.data.fill_(float("nan"))
    env.invalidate_outputs()
    env.step(a, autoreset=True)
    assert not torch.isnan(env.obs).any()
    env.close()

    off = BatchedDroneEnv(w, neighbors_num=10, reuse_obs=False)
    off.observe()
    off.step(a, autoreset=True)
    assert not _nan_left_after_step(off, a)
    off.close()


def test_caller_outputs_write_in_full():
    E, N = 64, 64
    w = synthetic_world(E, N, (50.0, 50.0, 10.0))
    env = BatchedDroneEnv(w, neighbors_num=10)
    env.observe()
    a = torch.from_numpy(synthetic_actions(E, N, 0)).float().cuda()
    o = torch.full_like(env.obs, float("nan"))
    c = torch.full_like(env.vo_count, -7)
    env.step_policy(a, obs_out=o, cnt_out=c)
    assert not torch.isnan(o).any() and int(c.min()) >= 0
    # writing into the env's own obs memory through another tensor ends the promise for the own pair
    env.observe(obs_out=env.obs.view(E, N, env.W), cnt_out=c)
    assert env._obs_ver is None
    env.close()


def test_step_ex_null_prev_is_full_write():
    """The C-ABI with prev_vo_count = NULL writes every byte, whatever the buffer held."""
    E, N = 8, 64
    env = BatchedDroneEnv(synthetic_world(E, N, (50.0, 50.0, 10.0)), neighbors_num=10, reuse_obs=False)
    env.observe()
    a = torch.from_numpy(synthetic_actions(E, N, 0)).cuda()
    env.obs.fill_(float("nan"))
    args = _lib.StepArgs()
    args.actions = a.data_ptr(); args.action_dtype = _lib.RVO3D_F64; args.policy = 0; args.autoreset = 1
    args.obs = env.obs.data_ptr(); args.vo_count = env.vo_count.data_ptr(); args.reward = env.reward.data_ptr()
    args.done = env.done.data_ptr(); args.info = env.info.data_ptr(); args.finish = env.finish.data_ptr()
    args.reset_mask = env.reset_mask.data_ptr(); args.prev_vo_count = None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().rvo3d_step_ex(env._h, C.byref(args), stream), "rvo3d_step_ex")
    torch.cuda.synchronize()
    assert not torch.isnan(env.obs).any()
    env.close()
