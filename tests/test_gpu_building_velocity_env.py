"""BuildingObsEnv(building_velocity=True) - observation rows that carry the nearest buildings as eight floats, velocity
and closing-time urgency at the relative velocity included (rvo3d_building_rows_moving) - against rows widened by hand
from the env's own dense pair, its state, device_buildings() and the motion's tensors through the plain-Python
restatement; and the trainer and the evaluator on those rows.
5 envs x 8 drones, nm = 10, a set of 6 buildings per env on a small map, k = 3: W = 126, state_dim = 36."""
import numpy as np
import pytest
import torch

from rvo3d_amd import BuildingObsEnv, synthetic_actions, synthetic_patrols, synthetic_world
from rvo3d_amd.policy import mlp_ac, multi_ppo, post_train
from rvo3d_amd.policy.policy_step import KernelPolicyStep
from building_rows_moving_ref import building_rows_moving_ref

pytestmark = pytest.mark.gpu
E, N, NM, K = 5, 8, 10, 3
MAP = (7.0, 7.0, 4.0)   # small: the drones meet and every building is near
RADIUS = 0.2


def world(seed=21):
    return synthetic_world(E, N, MAP, n_points=2, nb=6, seed=seed, min_sep=1.0, per_env_buildings=True)


def make(k=K, w=None):
    return BuildingObsEnv(world() if w is None else w, neighbors_num=NM, building_rows=k, building_velocity=True, radius=RADIUS)


def same(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def hand_widened(env, motion):
    """(the wide rows the restatement gives for the env's state now, its tally)"""
    st = env.get_state()
    bld, cnt = env.device_buildings()
    m = None if motion is None else tuple(t.cpu().numpy() for t in (motion.ends, motion.speed, motion.leg))
    rows, _, tally, _ = building_rows_moving_ref(st["pos"].cpu().numpy(), st["vel"].cpu().numpy(), RADIUS, bld.cpu().numpy(), K,
                                                 m, 1.0 if motion is None else motion.dt,
                                                 building_counts=None if cnt is None else cnt.cpu().numpy())
    dense = env._dense
    return torch.cat([dense[..., :12], torch.from_numpy(rows).cuda().view(E, N, 8 * K), dense[..., 12:]], dim=-1), tally


def test_attributes():
    env = make()
    assert (env.W, env.state_dim, env.W_dense) == (12 + 8 * K + 9 * NM, 12 + 8 * K, 12 + 9 * NM) == (126, 36, 102)
    assert tuple(env.obs.shape) == (E, N, 126) and env.building_velocity
    plain = BuildingObsEnv(world(), neighbors_num=NM, building_rows=K)
    assert (plain.W, plain.state_dim) == (120, 30) and not plain.building_velocity
    env.close(); plain.close()


def test_every_observation_equals_the_rows_widened_by_hand():
    """10 auto-resetting steps with a motion attached: after every step obs is the hand-widened twin.  Then the motion is
    detached: the next observation has zero velocity columns and the static urg.  Attached again - no new env -, the
    velocities are back."""
    env = make()
    motion = synthetic_patrols(env.world, seed=3, speed=(0.3, 1.5), span=6.0)
    env.attach_building_motion(motion)
    env.reset()
    o, _ = env.observe()
    hand, _ = hand_widened(env, motion)
    assert same(o, hand)
    total = dict(kept=0, moving=0, arrival=0, urg_differs=0, zero_to_positive=0)
    for t in range(10):
        a = synthetic_actions(E, N, t, seed=5) * 2.0
        o = env.step(a, autoreset=True)[0]
        hand, tally = hand_widened(env, motion)
        assert same(o, hand), t
        for n in total:
            total[n] += int(tally[n])
    print(total)
    assert min(total.values()) > 0, total
    b8 = o[..., 12:36].view(E, N, K, 8)
    assert bool(b8[..., 6:].any())
    # detached: every building stands
    env.attach_building_motion(None)
    o, _ = env.observe()
    hand, tally = hand_widened(env, None)
    assert same(o, hand) and tally["kept"] > 0 and tally["moving"] == 0
    b8 = o[..., 12:36].view(E, N, K, 8)
    r6, _ = env.building_rows(K)
    assert same(b8[..., :6], r6) and not bool(b8[..., 6:].view(torch.int32).any())
    # new sets and a new motion on the same env
    w2 = world(seed=22)
    env.set_env_buildings(w2.buildings, w2.building_counts)
    o, _ = env.observe()
    assert same(o, hand_widened(env, None)[0])
    motion2 = synthetic_patrols(w2, seed=4, speed=(0.3, 1.5), span=6.0)
    env.attach_building_motion(motion2)
    o = env.step(synthetic_actions(E, N, 11, seed=5) * 2.0, autoreset=True)[0]
    hand, tally = hand_widened(env, motion2)
    assert same(o, hand) and tally["moving"] > 0 and bool(o[..., 12:36].view(E, N, K, 8)[..., 6:].any())
    env.close()


def test_trainer_and_evaluator_on_rows_of_eight():
    """One multi_ppo epoch of 8 steps in mode "mlp" and one post_train(fused=True, policy_kernel="mlp_x3") on the env with a
    motion attached, mlp_ac(126): they run, and the buffer's first observation slot is env.obs of that step."""
    env = make()
    env.attach_building_motion(synthetic_patrols(env.world, seed=3, speed=(0.3, 1.5), span=6.0))
    torch.manual_seed(1)
    ac = mlp_ac(env.W).cuda()
    assert env.W == 126
    tr = multi_ppo(env, ac, steps_per_epoch=8, max_ep_len=50, train_pi_iters=1, train_v_iters=1, amp=True, seed=3)
    assert tr._fused_mode() == "mlp"
    assert tuple(tr.buf.obs.shape) == (9, E, N, 126)
    env.reset()
    first = env.observe()[0].clone()
    before = [q.detach().clone() for q in ac.parameters()]
    assert np.isfinite(tr.collect(final_reset=False))
    assert tr.buf.ptr == 8
    assert same(tr.buf.obs[0], first) and bool(first[..., 12:36].any())
    assert bool(tr.buf.obs[..., 12:36].reshape(9, E, N, K, 8)[..., 6:].any())   # velocities reach the buffer
    tr.update(tr.buf.get())
    assert any(not torch.equal(x, y) for x, y in zip(before, ac.parameters()))
    assert all(bool(torch.isfinite(q).all()) for q in ac.parameters())
    pt = post_train(env, num_episodes=2 * E, max_ep_len=10, acceler_vel=1.0, inf_print=False, std_factor=0.5, fused=True,
                    policy_kernel="mlp_x3", seed=11, poll_every=4)
    got = pt.policy_test(policy=ac)
    assert got["episodes"] == 2 * E and (pt.records["rec_len"] > 0).all()
    env.close()


def test_rows_wider_than_the_kernels_are_refused_as_before():
    """k = 4 rows of eight: W = 134 > 126.  The kernel modes refuse it with the message they have for every model that does
    not fit; the trainer falls back to a library-GEMM path."""
    env = make(k=4)
    assert (env.W, env.state_dim) == (134, 44)
    torch.manual_seed(1)
    ac = mlp_ac(env.W).cuda()
    for kind in ("mlp", "mlp_x3"):
        assert not KernelPolicyStep.fits(ac, kind, env.W)
        with pytest.raises(ValueError, match=r"needs an MLP\(256, 256\) actor-critic on the env's observation width"):
            KernelPolicyStep(ac, kind, env.W, E * N, option=f"rollout mode {kind!r}", state_dim=env.state_dim)
    tr = multi_ppo(env, ac, steps_per_epoch=4, max_ep_len=50, train_pi_iters=1, train_v_iters=1, amp=True, seed=3)
    assert tr._fused_mode() not in KernelPolicyStep.KINDS
    pt = post_train(env, num_episodes=1, max_ep_len=5, inf_print=False, fused=True, policy_kernel="mlp_x3")
    with pytest.raises(ValueError, match=r"policy_kernel='mlp_x3' needs an MLP\(256, 256\)"):
        pt.policy_test(policy=ac)
    env.close()
