"""The three entry points behind the fused evaluation loop, each against a restatement written here:
rvo3d_eval_action against the torch expression of the unfused loop (rvo3d_amd/policy/post_train.py), bit for bit;
rvo3d_eval_account against the bookkeeping of post_train.policy_test (train/policy/post_train.py:78-105) in numpy;
rvo3d_observe_envs against a full rvo3d_observe on a twin env in the same state."""
import ctypes as C

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, _lib, synthetic_actions, synthetic_world

pytestmark = pytest.mark.gpu
INVALID = -1


def p(t):
    return C.c_void_p(t.data_ptr())


def bits(t):
    """The tensor's bytes (NaN-aware, sign-of-zero-aware equality)."""
    return t.contiguous().view(torch.uint8).cpu().numpy()


def world(E, N):
    L = 6 + 2.0 * np.sqrt(N)
    return synthetic_world(E, N, (L, L, 6.0), n_points=2, seed=11)


# ---- rvo3d_eval_action -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N", [(5, 3), (2, 64), (3, 100)])
def test_eval_action_is_the_unfused_loops_torch_expression(E, N):
    env = BatchedDroneEnv(world(E, N))
    rng = np.random.default_rng(100 * E + N)
    vel = rng.uniform(-2, 2, (E, N, 3))
    vel[0, 0] = [0.0, -0.0, 1e-300]
    env.set_state(vel=vel)
    a = rng.uniform(-1.3, 1.3, (E, N, 3)).astype(np.float32)
    flat = a.reshape(-1)
    ties = np.array([0.125, -0.125, 0.375, 0.625, -0.875, 1.125, 0.005, -0.015, 0.045], np.float32)  # a * 100 ends in .5
    assert np.all((ties * np.float32(100.0)) % 1 == 0.5)
    flat[:len(ties)] = ties
    flat[len(ties):2 * len(ties)] = np.round(flat[len(ties):2 * len(ties)], 2)    # already rounded
    flat[2 * len(ties)] = 0.0
    flat[2 * len(ties) + 1] = -0.0
    at = torch.from_numpy(a).cuda()
    velt = torch.from_numpy(vel).cuda()
    for acc in (1.0, 0.5, 0.3):
        a_inc = torch.round(at * 100.0) / torch.full_like(at, 100.0)
        want = (torch.as_tensor(acc, dtype=torch.float32, device="cuda") * a_inc).double() + velt
        got = env.eval_action(at, acc)
        assert got.dtype == torch.float64 and tuple(got.shape) == (E, N, 3)
        assert np.array_equal(bits(got), bits(want)), acc
    assert env.eval_action(at, 1.0).data_ptr() == got.data_ptr()      # a persistent buffer
    Lb = _lib.lib()
    assert Lb.rvo3d_eval_action(env._h, None, 1.0, p(got), None) == INVALID
    assert Lb.rvo3d_eval_action(env._h, p(at), 1.0, None, None) == INVALID
    assert Lb.rvo3d_eval_action(None, p(at), 1.0, p(got), None) == INVALID
    env.close()


# ---- rvo3d_eval_account ------------------------------------------------------------------------------------------
CALLS, MAX_EP_LEN, QUOTA = 6, 3, 2
NAMES = ("ep_len", "ep_ret", "speed_sum", "counted", "rec_len", "rec_ret", "rec_speed", "rec_step", "rec_flags",
         "remaining", "ended")


def account_inputs(E, N, seed):
    """Per call: velocities, rewards (NaN / +-inf among r[0]), and flag bytes whose density follows N: an env's drones
    all arrive in about half of the steps, all finish in about 0.3 of them, and some drone collides in about 0.15."""
    rng = np.random.default_rng(seed)
    p_all, p_fin, p_done = 0.5 ** (1.0 / N), 0.3 ** (1.0 / N), 1.0 - 0.85 ** (1.0 / N)
    calls = []
    for t in range(CALLS):
        rew = rng.normal(0, 3, (E, N)).astype(np.float32)
        odd = rng.uniform(size=E)
        rew[odd < 0.08, 0] = np.nan
        rew[(odd >= 0.08) & (odd < 0.14), 0] = np.inf
        rew[(odd >= 0.14) & (odd < 0.2), 0] = -np.inf
        calls.append(dict(vel=rng.uniform(-2, 2, (E, N, 3)), rew=rew,
                          done=(rng.uniform(size=(E, N)) < p_done).astype(np.uint8),
                          finish=(rng.uniform(size=(E, N)) < p_fin).astype(np.uint8) * rng.integers(1, 255, (E, N), dtype=np.uint8),
                          info=(rng.uniform(size=(E, N)) < p_all).astype(np.uint8)))
    return calls


def account_reference(E, N, calls):
    """post_train.policy_test's bookkeeping (:78-105), env by env."""
    s = dict(ep_len=np.zeros(E, np.int32), ep_ret=np.zeros(E), speed_sum=np.zeros(E), counted=np.zeros(E, np.int32),
             rec_len=np.zeros((E, QUOTA), np.int32), rec_ret=np.zeros((E, QUOTA)), rec_speed=np.zeros((E, QUOTA)),
             rec_step=np.zeros((E, QUOTA), np.int64), rec_flags=np.zeros((E, QUOTA), np.uint8),
             remaining=np.array([E * QUOTA], np.int32), ended=np.zeros(E, np.uint8))
    seen, per_call = set(), []
    with np.errstate(invalid="ignore"):
        for t, c in enumerate(calls):
            for e in range(E):
                v = c["vel"][e]
                s["speed_sum"][e] += np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).sum() / N
                s["ep_ret"][e] += np.float64(c["rew"][e, 0])
                ln = s["ep_len"][e] + 1
                any_done, all_fin, all_info = c["done"][e].any(), c["finish"][e].all(), c["info"][e].all()
                timeout = ln == MAX_EP_LEN
                ended = any_done or timeout or all_fin
                if ended and s["counted"][e] < QUOTA:
                    k = s["counted"][e]
                    s["rec_len"][e, k], s["rec_ret"][e, k] = ln, s["ep_ret"][e]
                    s["rec_speed"][e, k], s["rec_step"][e, k] = s["speed_sum"][e] / ln, 1000 + t
                    s["rec_flags"][e, k] = 1 * all_info + 2 * all_fin + 4 * any_done + 8 * timeout
                    s["counted"][e] += 1
                    s["remaining"][0] -= 1
                    seen.add(int(s["rec_flags"][e, k]))
                elif ended:
                    seen.add("past quota")
                if ended:
                    s["ep_len"][e], s["ep_ret"][e], s["speed_sum"][e] = 0, 0.0, 0.0
                else:
                    s["ep_len"][e] = ln
                s["ended"][e] = ended
            per_call.append((s["ended"].copy(), int(s["remaining"][0])))
    return s, seen, per_call


def account_on_device(env, calls):
    E, dev = env.E, env.device
    dt = dict(ep_len=torch.int32, ep_ret=torch.float64, speed_sum=torch.float64, counted=torch.int32, rec_len=torch.int32,
              rec_ret=torch.float64, rec_speed=torch.float64, rec_step=torch.int64, rec_flags=torch.uint8,
              remaining=torch.int32, ended=torch.uint8)
    t = {k: torch.zeros((E, QUOTA) if k.startswith("rec_") else (1,) if k == "remaining" else (E,), dtype=dt[k], device=dev)
         for k in NAMES}
    t["remaining"].fill_(E * QUOTA)
    t["ended"].fill_(77)       # (written in full by every call)
    bufs = _lib.EvalBufs(**{k: v.data_ptr() for k, v in t.items()})
    per_call = []
    for i, c in enumerate(calls):
        env.set_state(vel=c["vel"])
        dev_in = [torch.from_numpy(c[k]).cuda() for k in ("rew", "done", "info", "finish")]
        _lib.check(_lib.lib().rvo3d_eval_account(env._h, *[p(x) for x in dev_in], MAX_EP_LEN, QUOTA, 1000 + i,
                                                 C.byref(bufs), env._stream()), "rvo3d_eval_account")
        per_call.append((t["ended"].cpu().numpy().copy(), int(t["remaining"].item())))
    return {k: v.cpu().numpy() for k, v in t.items()}, per_call, (bufs, dev_in)


@pytest.mark.parametrize("E,N", [(37, 5), (16, 64), (9, 100), (3, 300)])
def test_eval_account_is_policy_tests_bookkeeping(E, N):
    calls = account_inputs(E, N, seed=7 * E + N)
    want, seen, want_calls = account_reference(E, N, calls)
    if E >= 9:  # the inputs reach every branch: each flag bit, an env past its quota, a non-finite return on record
        flags = [f for f in seen if f != "past quota"]
        assert "past quota" in seen and all(any(f & b for f in flags) for b in (1, 2, 4, 8)), seen
        assert not np.isfinite(want["rec_ret"]).all()
        assert want_calls[1][1] > 0     # (the quota is not used up at once: `remaining` is compared on its way down)
    env = BatchedDroneEnv(world(E, N))
    got, got_calls, (bufs, dev_in) = account_on_device(env, calls)
    for (ea, ra), (eb, rb) in zip(got_calls, want_calls):
        assert np.array_equal(ea, eb) and ra == rb
    for k in NAMES:
        if k in ("speed_sum", "rec_speed"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
        else:   # every integer, flag and byte, and ep_ret / rec_ret (the same sequential float64 adds), NaN == NaN
            assert got[k].dtype == want[k].dtype, k
            assert np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f"), k
    again, again_calls, _ = account_on_device(env, calls)
    for k in NAMES:
        assert got[k].tobytes() == again[k].tobytes(), k
    assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(got_calls, again_calls))
    Lb = _lib.lib()
    args = [p(x) for x in dev_in]
    assert Lb.rvo3d_eval_account(env._h, None, *args[1:], MAX_EP_LEN, QUOTA, 0, C.byref(bufs), None) == INVALID
    assert Lb.rvo3d_eval_account(env._h, *args, MAX_EP_LEN, QUOTA, 0, None, None) == INVALID
    assert Lb.rvo3d_eval_account(env._h, *args, MAX_EP_LEN, 0, 0, C.byref(bufs), None) == INVALID
    hole = _lib.EvalBufs.from_buffer_copy(bufs)
    hole.rec_step = None
    assert Lb.rvo3d_eval_account(env._h, *args, MAX_EP_LEN, QUOTA, 0, C.byref(hole), None) == INVALID
    env.close()


# ---- rvo3d_observe_envs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N", [(7, 3), (5, 64), (3, 100), (2, 130)])
def test_observe_envs_rewrites_the_masked_envs_only(E, N):
    w = world(E, N)
    env, twin = BatchedDroneEnv(w), BatchedDroneEnv(w)
    act = lambda t: torch.from_numpy(synthetic_actions(E, N, t, seed=3 * N)).cuda()
    for e_ in (env, twin):
        e_.reset()
        e_.observe()
        for t in range(2):
            e_.step(act(t))
    rng = np.random.default_rng(N)
    random_mask = rng.integers(0, 2, E).astype(np.uint8)
    random_mask[:2] = [1, 0]
    for t, mask in enumerate([random_mask * 3, np.zeros(E, np.uint8), np.ones(E, np.uint8)]):
        if t < 2:
            # what the unmasked rows must keep is unlike anything an observation writes (the in-place ops also tell
            # the env that its pair is no longer the library's: the next step writes in full)
            env.obs.add_(1000.0)
            env.vo_count.add_(50)
        before_o, before_c = env.obs.clone(), env.vo_count.clone()
        m = torch.from_numpy(mask).cuda()
        o, c = env.observe_envs(m)
        assert o.data_ptr() == env.obs.data_ptr() and c.data_ptr() == env.vo_count.data_ptr()
        full_o, full_c = twin.observe()
        for e in range(E):
            src_o, src_c = (full_o, full_c) if mask[e] else (before_o, before_c)
            assert np.array_equal(bits(o[e]), bits(src_o[e])), (t, e)
            assert np.array_equal(bits(c[e]), bits(src_c[e])), (t, e)
        # (t == 2: every row comes from the library again and the pair was the step's own - the step below leaves out
        # the zeros the buffer holds, and must still agree with the twin's)
        assert (env._obs_ver is not None) == (t == 2)
        outs_a = env.step(act(2 + t))
        outs_b = twin.step(act(2 + t))
        for x, y in zip(outs_a, outs_b):
            assert np.array_equal(bits(x), bits(y)), t
        sa, sb = env.get_state(), twin.get_state()
        for k in sa:
            assert np.array_equal(bits(sa[k]), bits(sb[k])), (t, k)
    Lb = _lib.lib()
    so, sc = env._scratch
    assert Lb.rvo3d_observe_envs(env._h, None, p(env.obs), p(env.vo_count), p(so), p(sc), None) == INVALID
    assert Lb.rvo3d_observe_envs(env._h, p(m), p(env.obs), p(env.vo_count), None, p(sc), None) == INVALID
    assert Lb.rvo3d_observe_envs(env._h, p(m), p(env.obs), p(env.vo_count), p(so), None, None) == INVALID
    env.close(); twin.close()
