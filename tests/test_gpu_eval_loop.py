"""The fused evaluation loop (rvo3d_amd.policy.post_train, fused=True): the reference's policy_test per env with the
episodes accounted for on the device - against the reference's own runs (tests/golden/post_train_*.npz), against the
unfused loop where the two must agree, and against single-env runs where only the fused loop keeps the envs apart."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from golden_util import load
from rvo3d_amd import BatchedDroneEnv, World, _lib, synthetic_world
from rvo3d_amd.policy import mlp_ac, post_train, rnn_ac
from test_gpu_parity import _TablePolicy, world_of

pytestmark = pytest.mark.gpu
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(_ROOT, "tests", "golden")
POST_TRAIN = sorted(f for f in os.listdir(GOLDEN) if f.startswith("post_train_"))


@pytest.mark.parametrize("name", POST_TRAIN)
def test_fused_post_train_matches_the_references_policy_test(name):
    """The assertions of test_post_train_matches_the_references_policy_test, on the fused loop."""
    fx = load(os.path.join(GOLDEN, name))
    env = BatchedDroneEnv(world_of(fx), neighbors_num=10, env_train=bool(fx["env_train"]))
    pt = post_train(env, num_episodes=int(fx["num_episodes"]), max_ep_len=int(fx["max_ep_len"]),
                    acceler_vel=1.0, inf_print=False, std_factor=1e-5, fused=True)
    got = pt.policy_test(policy=_TablePolicy(fx["table"], [0]), policy_name="scripted")
    env.close()
    arrived = fx["ep_arrived"].astype(bool)
    assert got["episodes"] == int(fx["num_episodes"]) == len(fx["ep_len"])
    assert got["ep_len"] == fx["ep_len"][arrived].tolist()
    np.testing.assert_allclose(got["speed"], fx["ep_speed"], rtol=1e-12)
    assert got["success_rate"] == pytest.approx(float(fx["success_rate"]), abs=1e-4)  # printed as xx.xx%
    assert got["success_rate"] == fx["ep_finished"].mean()
    for k in ("mean_len", "std_len", "average_speed", "std_speed"):
        assert got[k] == float(fx[k]), k
    # the records behind the result: one per episode, flags as the reference saw them
    rec = pt.records
    order = np.argsort(rec["rec_step"][0])
    assert rec["rec_len"][0][order].tolist() == fx["ep_len"].tolist()
    assert ((rec["rec_flags"][0][order] & 4) != 0).tolist() == fx["ep_collided"].astype(bool).tolist()
    assert ((rec["rec_flags"][0][order] & 1) != 0).tolist() == arrived.tolist()


def test_fused_and_unfused_loops_agree_on_a_scripted_policy():
    """E = 3 on the action table (a policy that does not look at its observation): both loops count the same episodes,
    in the same order; the fused result does not depend on how often the host looks."""
    fx = load(os.path.join(GOLDEN, "post_train_world_4_eval.npz"))
    E, quota = 3, 2
    starts = np.concatenate([[0], np.cumsum(fx["ep_len"])])[:E].tolist()

    def run(**kw):
        env = BatchedDroneEnv(world_of(fx, E), neighbors_num=10, env_train=False)
        pt = post_train(env, num_episodes=E * quota - 1, max_ep_len=int(fx["max_ep_len"]), acceler_vel=1.0,
                        inf_print=False, **kw)
        got = pt.policy_test(policy=_TablePolicy(fx["table"], starts))
        env.close()
        return got

    unfused, fused1, fused7 = run(), run(fused=True, poll_every=1), run(fused=True, poll_every=7)
    assert fused1 == fused7
    assert unfused["episodes"] == fused1["episodes"] == E * quota
    for k in ("ep_len", "ep_ret", "success_rate", "mean_len", "std_len", "average_speed", "std_speed"):
        assert fused1[k] == unfused[k], k
    np.testing.assert_allclose(fused1["speed"], unfused["speed"], rtol=1e-12)   # (same order: elementwise)


class _ObsPolicy:
    """Stand-in policy that looks at its observation, elementwise only (no reduction: a row's action cannot depend on
    the batch): steer the velocity (columns 3..5) towards the desired one (8..10) and along the first velocity-obstacle
    row (12..14), clamped to +-1."""

    def __init__(self):
        self.max_cnt = torch.zeros((), dtype=torch.int32, device="cuda")

    def eval(self):
        return self

    def step_tensors(self, obs, std_factor=1):
        x, cnt = obs
        self.max_cnt = torch.maximum(self.max_cnt, cnt.max())
        a = torch.clamp(0.6 * (x[:, 8:11] - x[:, 3:6]) + 0.4 * x[:, 12:15], -1.0, 1.0)
        return a, None, None


def test_fused_envs_do_not_depend_on_each_other():
    """Three different small worlds in one E = 3 env, a policy that looks at its observation: every env's episodes are
    those of the same world evaluated alone (the reference's loop, E = 1).  Only the envs that were reset are re-observed;
    the unfused loop re-observes all of them and is not asserted either way (on this world its returns differ)."""
    N, quota, max_ep_len = 6, 2, 25
    w = synthetic_world(3, N, (7.0, 7.0, 4.0), n_points=2, seed=21, min_sep=1.0)

    def run(world):
        env = BatchedDroneEnv(world, neighbors_num=10, env_train=True)
        pol = _ObsPolicy()
        pt = post_train(env, num_episodes=world.shape[0] * quota, max_ep_len=max_ep_len, acceler_vel=1.0,
                        inf_print=False, fused=True, poll_every=5)
        pt.policy_test(policy=pol)
        env.close()
        return pt.records, int(pol.max_cnt.item())

    rec3, max_cnt = run(w)
    print("lengths", rec3["rec_len"].tolist(), "flags", rec3["rec_flags"].tolist(), "largest vo_count", max_cnt)
    assert max_cnt > 0      # velocity-obstacle rows occurred: the observation with and without the action differ
    lens = rec3["rec_len"]
    assert len({tuple(r) for r in lens.tolist()}) > 1   # the envs end their episodes at different steps
    for e in range(3):
        rec1, _ = run(World(w.waypoints[e:e + 1].copy(), w.n_points[e:e + 1].copy(), w.map_size, w.buildings))
        for k in ("rec_len", "rec_flags", "rec_ret", "rec_step"):
            assert np.array_equal(rec3[k][e], rec1[k][0], equal_nan=k == "rec_ret"), (e, k)
        np.testing.assert_allclose(rec3["rec_speed"][e], rec1["rec_speed"][0], rtol=1e-12)


def _mlp_policy(env):
    torch.manual_seed(3)
    return mlp_ac(env.W).cuda()


@pytest.mark.parametrize("kernel", ["mlp_x3", "mlp"])
def test_kernel_policy_in_both_loops(kernel):
    """policy_kernel: the whole policy step as one kernel, noise from (seed, call number) - the same actions in both
    loops, so with E = 1 the same episodes; the first call is the entry point's own output for step 0."""
    fx = load(os.path.join(GOLDEN, "post_train_world_8_train.npz"))
    got = {}
    for fused in (False, True):
        env = BatchedDroneEnv(world_of(fx), neighbors_num=10, env_train=True)
        ac = _mlp_policy(env)
        pt = post_train(env, num_episodes=3, max_ep_len=12, acceler_vel=1.0, inf_print=False, std_factor=0.5,
                        fused=fused, policy_kernel=kernel, seed=11)
        got[fused] = pt.policy_test(policy=ac)
        env.close()
    assert got[True]["episodes"] == got[False]["episodes"] == 3
    for k in ("ep_len", "ep_ret", "success_rate", "mean_len", "std_len", "average_speed", "std_speed"):
        assert got[True][k] == got[False][k], k
    np.testing.assert_allclose(got[True]["speed"], got[False]["speed"], rtol=1e-12)

    # the first policy call against a direct call of the entry point
    env = BatchedDroneEnv(world_of(fx), neighbors_num=10, env_train=True)
    ac = _mlp_policy(env)
    pt = post_train(env, num_episodes=3, max_ep_len=12, inf_print=False, std_factor=0.5, policy_kernel=kernel, seed=11)
    act_fn = pt.load_policy(ac, pt.std_factor)
    env.reset()
    obs, cnt = env.observe()
    first = act_fn(obs.view(-1, env.W), cnt.view(-1)).clone()
    second = act_fn(obs.view(-1, env.W), cnt.view(-1)).clone()
    mb = ac.mlp_blob("bf16" if kernel == "mlp" else "x3")
    L = _lib.lib()
    fn = L.rvo3d_policy_mlp_sample if kernel == "mlp" else L.rvo3d_policy_mlp_x3_sample
    p = lambda t: C.c_void_p(t.data_ptr())
    rows = env.E * env.N
    out = [torch.empty((rows, 3), device="cuda"), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")]
    for step, want in ((0, first), (1, second)):
        _lib.check(fn(p(mb["blob"]), env.W, p(obs), env.W, rows, p(cnt), 12, 9, 1 if mb["tanh"] else 0, p(ac.log_std), 0.5,
                      11, step, *[p(x) for x in out], None, None, env._stream()), "policy sample")
        assert torch.equal(out[0].view(torch.int32), want.view(torch.int32)), step
    assert not torch.equal(first, second)    # (the call number is the noise step)
    env.close()


def test_kernel_policy_needs_the_mlp_actor_critic():
    fx = load(os.path.join(GOLDEN, "post_train_world_8_train.npz"))
    env = BatchedDroneEnv(world_of(fx), neighbors_num=10)

    class Space:
        shape = (3,)
    rnn = rnn_ac(None, Space(), 12, 9, 64, (64, 64), (64, 64), torch.nn.ReLU, torch.nn.Tanh, torch.nn.Identity,
                 use_gpu=False, rnn_mode="biGRU").cuda()
    for fused in (False, True):
        pt = post_train(env, num_episodes=1, max_ep_len=5, inf_print=False, fused=fused, policy_kernel="mlp")
        with pytest.raises(ValueError, match="policy_kernel"):
            pt.policy_test(policy=rnn)
    with pytest.raises(ValueError):
        post_train(env, policy_kernel="gemm")
    env.close()


def test_fused_loop_raises_the_domain_error_at_the_next_poll():
    """env_train=False: two drones that approach inside r + mr (0.2 + 0.2; 0.3 m apart, closing at 0.2 m/s) are where the
    reference's evaluator raises "math domain error" (vel_obs3D.py:13).  The state is put in place through set_state behind
    the loop's first reset; the fused loop raises at its next poll - within poll_every steps."""
    wp = np.array([[[[5.0, 5.0, 2.0], [9.0, 5.0, 2.0]], [[5.3, 5.0, 2.0], [1.0, 5.0, 2.0]]]])
    env = BatchedDroneEnv(World(wp, np.full((1, 2), 2, np.int32), np.array([10.0, 10.0, 5.0]), np.zeros((0, 4))),
                          neighbors_num=10, env_train=False)
    plain_reset = env.reset
    steps = []

    def reset_into_the_shell(env_mask=None):
        plain_reset(env_mask)
        if env_mask is None:
            env.set_state(vel=np.array([[[0.1, 0.0, 0.0], [-0.1, 0.0, 0.0]]]))

    class _Still(_TablePolicy):      # a = 0: the action is the velocity on file
        def step_tensors(self, obs, std_factor=1):
            steps.append(1)
            return super().step_tensors(obs, std_factor)

    env.reset = reset_into_the_shell
    poll_every = 4
    pt = post_train(env, num_episodes=2, max_ep_len=30, acceler_vel=1.0, inf_print=False, fused=True,
                    poll_every=poll_every)
    with pytest.raises(ValueError, match="math domain error"):
        pt.policy_test(policy=_Still(np.zeros((1, 2, 3), np.float32), [0]))
    assert len(steps) == poll_every
    env.close()
