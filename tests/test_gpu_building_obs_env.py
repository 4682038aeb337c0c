"""BuildingObsEnv - the env whose observation rows carry the nearest buildings - against a plain twin env whose dense
output is widened by hand, and the policy step, the trainer and the evaluator on the wider rows.
4 envs x 8 drones, nm = 10, a set of 6 buildings per env, k = 4: W = 126, state_dim = 36."""
import ctypes as C

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, BuildingObsEnv, _lib, synthetic_actions, synthetic_world
from rvo3d_amd.policy import mlp_ac, multi_ppo, post_train, rnn_ac

pytestmark = pytest.mark.gpu
E, N, NM, K = 4, 8, 10, 4
MAP = (7.0, 7.0, 4.0)   # small: the drones meet (velocity-obstacle rows from the first step on) and every building is near


def world(envs=E, seed=21):
    return synthetic_world(envs, N, MAP, n_points=2, nb=6, seed=seed, min_sep=1.0, per_env_buildings=True)


def pair(w=None):
    w = world() if w is None else w
    return BuildingObsEnv(w, neighbors_num=NM, building_rows=K), BatchedDroneEnv(w, neighbors_num=NM)


def widen(twin, dense):
    """The twin's dense rows with the building rows of its current state spliced in behind the 12 proprio floats."""
    rows, _ = twin.building_rows(K)
    return torch.cat([dense[..., :12], rows.view(twin.E, twin.N, 6 * K), dense[..., 12:]], dim=-1)


def same(a, b):
    """Bit for bit (NaN-safe)."""
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def same_outputs(env, twin):
    return all(same(getattr(env, n), getattr(twin, n)) for n in ("reward", "done", "info", "finish"))


class Space:
    shape = (3,)


def test_attributes():
    env, twin = pair()
    assert (env.W, env.state_dim, env.W_dense) == (12 + 6 * K + 9 * NM, 12 + 6 * K, 12 + 9 * NM) == (126, 36, 102)
    assert tuple(env.obs.shape) == (E, N, 126) and twin.W == 102 and not hasattr(twin, "state_dim")
    with pytest.raises(ValueError):
        BuildingObsEnv(world(), neighbors_num=NM, building_rows=9)
    env.close(); twin.close()


def test_every_observation_equals_the_twins_widened_by_hand():
    env, twin = pair()
    env.reset(); twin.reset()
    o, c = env.observe()
    do, dc = twin.observe()
    assert same(o, widen(twin, do)) and same(c, dc)
    seen_buildings = seen_vo = False
    for t in range(4):        # the plain step
        a = synthetic_actions(E, N, t, seed=5) * 2.0
        o, c = env.step(a)[:2]
        do, dc = twin.step(a)[:2]
        assert same(o, widen(twin, do)) and same(c, dc) and same_outputs(env, twin), t
        seen_vo |= bool((c > 0).any())
    for t in range(4, 9):     # the auto-resetting step: a reset drone's rows are those of its reset state
        a = synthetic_actions(E, N, t, seed=5) * 2.0
        o, c = env.step(a, autoreset=True)[:2]
        do, dc = twin.step(a, autoreset=True)[:2]
        assert same(o, widen(twin, do)) and same(c, dc) and same_outputs(env, twin), t
        seen_buildings |= bool(o[..., 12:36].any())
        seen_vo |= bool((c > 0).any())
    slot_o = torch.full((E, N, env.W), -7.0, device="cuda")   # step_policy into a caller's slot
    slot_c = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
    own = env.obs.clone()
    g = torch.Generator(device="cuda").manual_seed(4)
    for t in range(9, 13):
        a = torch.rand((E, N, 3), device="cuda", generator=g) * 2 - 1
        o, c = env.step_policy(a, autoreset=True, obs_out=slot_o, cnt_out=slot_c)[:2]
        do, dc = twin.step_policy(a, autoreset=True)[:2]
        assert o.data_ptr() == slot_o.data_ptr() and same(o, widen(twin, do)) and same(c, dc) and same_outputs(env, twin), t
        assert same(env.obs, own)   # the env's own tensor is not written
        seen_buildings |= bool(o[..., 12:36].any())
        seen_vo |= bool((c > 0).any())
    assert seen_buildings and seen_vo
    # observe_envs: envs 0 and 2 reset and re-observed; the others keep the dense row of their last observation and get
    # back the building floats of their (unchanged) state
    env.step(a * 0.5); twin.step(a * 0.5)
    mask = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device="cuda")
    env.reset(mask); twin.reset(mask)
    o, c = env.observe_envs(mask)
    do, dc = twin.observe_envs(mask)
    assert same(o, widen(twin, do)) and same(c, dc)
    env.close(); twin.close()


@pytest.mark.parametrize("entry", ["rvo3d_policy_mlp_sample", "rvo3d_policy_mlp_x3_sample"])
def test_mlp_kernels_take_the_wide_row_with_state_dim_36(entry):
    """With the env's vo_count and state_dim = 36 the kernels skip the column groups behind 36 + 9 * vo_count; the wide
    row keeps their promise (zeros there), so act / logp / val are those of a call without counts."""
    env, twin = pair()
    env.reset()
    env.observe()
    obs, cnt = env.step(synthetic_actions(E, N, 0, seed=5) * 2.0)[:2]
    assert bool((cnt > 0).any()) and bool(obs[..., 12:36].any())
    # the promise itself: zeros behind state_dim + 9 * vo_count
    cols = torch.arange(env.W, device="cuda")[None, None, :]
    assert not bool((obs * (cols >= (36 + 9 * cnt)[..., None])).any())
    torch.manual_seed(3)
    ac = mlp_ac(env.W).cuda()
    mb = ac.mlp_blob("bf16" if entry == "rvo3d_policy_mlp_sample" else "x3")
    assert mb is not None
    fn = getattr(_lib.lib(), entry)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rows = E * N

    def run(counts, state_dim):
        out = [torch.empty((rows, 3), device="cuda"), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")]
        _lib.check(fn(p(mb["blob"]), env.W, p(obs), env.W, rows, p(counts), state_dim, 9, 1 if mb["tanh"] else 0,
                      p(ac.log_std), 0.5, 11, 2, *[p(x) for x in out], None, None, env._stream()), entry)
        return out
    with_counts, without = run(cnt, env.state_dim), run(None, 0)
    for a, b, name in zip(with_counts, without, ("act", "logp", "val")):
        assert same(a, b), name
    env.close(); twin.close()


@pytest.mark.parametrize("graph", [False, True])
def test_trainer_rollouts_on_wide_rows(graph):
    """multi_ppo on the wide env picks the one-kernel MLP step; every stored observation is the twin's - stepped with the
    stored actions - widened by hand.  graph_rollout=True: the second epoch replays captured launches."""
    T = 4
    env, twin = pair()
    torch.manual_seed(1)
    ac = mlp_ac(env.W).cuda()
    tr = multi_ppo(env, ac, steps_per_epoch=T, max_ep_len=50, train_pi_iters=1, train_v_iters=1, amp=True, seed=3,
                   graph_rollout=graph)
    assert tr._fused_mode() == "mlp"
    assert tuple(tr.buf.obs.shape) == (T + 1, E, N, env.W)
    env.reset(); env.observe()
    twin.reset()
    do, dc = twin.observe()
    o = widen(twin, do)
    for epoch in range(2 if graph else 1):
        tr.buf.ptr = 0
        tr.collect(final_reset=False)
        buf = tr.buf
        assert same(buf.obs[0], o) and same(buf.cnt[0], dc), epoch
        for t in range(T):
            do, dc = twin.step_policy(buf.act[t], autoreset=True)[:2]
            o = widen(twin, do)
            assert same(buf.obs[t + 1], o) and same(buf.cnt[t + 1], dc), (epoch, t)
        assert bool(buf.obs[..., 12:36].any())
        if graph and not getattr(tr, "_graph_failed", False):
            assert (len(getattr(tr, "_graphs", {})) > 0) == (epoch >= 1)
    assert _lib.lib().rvo3d_rollout_set_step_counter(None) == 0
    env.close(); twin.close()


def test_evaluator_on_wide_rows():
    """post_train(fused=True, policy_kernel="mlp_x3", safety=True) on the wide env: two episodes per env; at E = 1 the
    fused and the unfused loop count the same episodes."""
    env = BuildingObsEnv(world(), neighbors_num=NM, building_rows=K)
    torch.manual_seed(3)
    ac = mlp_ac(env.W).cuda()
    pt = post_train(env, num_episodes=2 * E, max_ep_len=10, acceler_vel=1.0, inf_print=False, std_factor=0.5, fused=True,
                    policy_kernel="mlp_x3", safety=True, seed=11, poll_every=4)
    got = pt.policy_test(policy=ac)
    assert got["episodes"] == 2 * E and pt.safety["episodes"] == 2 * E
    assert (pt.records["rec_len"] > 0).all()
    env.close()
    res = {}
    for fused in (False, True):
        env1 = BuildingObsEnv(world(1), neighbors_num=NM, building_rows=K)
        pt = post_train(env1, num_episodes=2, max_ep_len=10, acceler_vel=1.0, inf_print=False, std_factor=0.5, fused=fused,
                        policy_kernel="mlp_x3", safety=True, seed=11, poll_every=3)
        res[fused] = (pt.policy_test(policy=ac), pt.safety)
        env1.close()
    for k in ("episodes", "ep_len", "ep_ret", "success_rate", "mean_len", "std_len", "average_speed", "std_speed"):
        assert res[True][0][k] == res[False][0][k], k
    for k in ("episodes", "min_min_sep", "min_min_bclear", "min_min_wall"):
        assert res[True][1][k] == res[False][1][k], k


def _rnn(state_dim):
    torch.manual_seed(2)
    return rnn_ac(None, Space(), state_dim, 9, 64, (64, 64), (64, 64), torch.nn.ReLU, torch.nn.Tanh, torch.nn.Identity,
                  use_gpu=False, rnn_mode="biGRU").cuda()


def test_reader_state_dim_must_be_the_envs():
    """A 12-float reader on the wide row (6k = 24 here; with k = 3 the rest would even divide by 9) is refused by the
    trainer and by the evaluator, with both numbers in the message; a 36-float reader trains on the torch path."""
    env, twin = pair()
    with pytest.raises(ValueError, match=r"state_dim=12.*state_dim=36"):
        multi_ppo(env, _rnn(12), steps_per_epoch=4)
    pt = post_train(env, num_episodes=1, max_ep_len=5, inf_print=False)
    with pytest.raises(ValueError, match=r"state_dim=12.*state_dim=36"):
        pt.load_policy(_rnn(12))
    with pytest.raises(ValueError, match=r"state_dim=36.*state_dim=12"):
        multi_ppo(twin, _rnn(36), steps_per_epoch=4)
    multi_ppo(twin, _rnn(12), steps_per_epoch=4)   # the plain pair is accepted as before
    ac = _rnn(36)
    tr = multi_ppo(env, ac, steps_per_epoch=4, max_ep_len=50, train_pi_iters=1, train_v_iters=1, seed=3)
    assert tr._fused_mode() == "direct"   # (the fused biGRU kernels stop at state_dim 16)
    env.reset(); env.observe()
    before = [q.detach().clone() for q in ac.parameters()]
    assert np.isfinite(tr.collect())
    tr.update(tr.buf.get())
    assert any(not torch.equal(a, b) for a, b in zip(before, ac.parameters()))
    assert all(bool(torch.isfinite(q).all()) for q in ac.parameters())
    env.close(); twin.close()


def test_a_building_next_to_a_drone_shows_in_its_row_alone():
    """Moving one building of env 1 next to drone 5 changes that drone's wide row and the policy's mean for it, and no
    other row's."""
    w = world()
    env = BuildingObsEnv(w, neighbors_num=NM, building_rows=K)
    env.reset()
    base = env.observe()[0].clone()
    pos = env.get_state()["pos"].cpu().numpy()
    b = np.array(w.buildings, dtype=np.float64).copy()
    far = b.copy()
    far[1, 0] = [-50.0, -50.0, 4.0, 0.5]          # first out of everybody's reach ...
    env.set_env_buildings(far, w.building_counts)
    o_far = env.observe()[0].clone()
    near = far.copy()
    near[1, 0] = [pos[1, 5, 0] + 0.6, pos[1, 5, 1], pos[1, 5, 2] + 1.0, 0.25]   # ... then next to drone 5 of env 1
    env.set_env_buildings(near, w.building_counts)
    o_near = env.observe()[0].clone()
    d = np.hypot(pos[1, :, 0] - near[1, 0, 0], pos[1, :, 1] - near[1, 0, 1])
    seen_by = set(np.flatnonzero(d <= 5.0).tolist())
    assert 5 in seen_by
    changed = (o_near.view(torch.int32) != o_far.view(torch.int32)).any(dim=-1).cpu().numpy()
    assert changed[1, 5] and set(np.flatnonzero(changed[1]).tolist()) <= seen_by
    assert not changed[[0, 2, 3]].any()
    assert same(o_near[..., :12], base[..., :12]) and same(o_near[..., 36:], base[..., 36:])   # only building floats move
    mine = [s for s in range(K) if o_near[1, 5, 12 + 6 * s:16 + 6 * s].tolist() == pytest.approx([0.6, 0.0, 1.0, 0.25])]
    assert len(mine) == 1 and o_near[1, 5, 12 + 6 * mine[0] + 5] == 0   # (a reset drone stands still: urg 0)
    # ... and in the policy's mean (dbg_mu of the one-kernel step), for the rows that changed alone
    torch.manual_seed(3)
    ac = mlp_ac(env.W).cuda()
    mb = ac.mlp_blob("x3")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rows = E * N

    def mu_of(obs):
        out = [torch.empty((rows, 3), device="cuda"), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")]
        mu = torch.empty((rows, 3), device="cuda")
        _lib.check(_lib.lib().rvo3d_policy_mlp_x3_sample(p(mb["blob"]), env.W, p(obs), env.W, rows, p(env.vo_count),
                                                         env.state_dim, 9, 1 if mb["tanh"] else 0, p(ac.log_std), 0.5, 11, 0,
                                                         *[p(x) for x in out], p(mu), None, env._stream()), "mlp_x3")
        return mu.view(E, N, 3)
    mu_far, mu_near = mu_of(o_far), mu_of(o_near)
    mu_changed = (mu_far.view(torch.int32) != mu_near.view(torch.int32)).any(dim=-1).cpu().numpy()
    assert mu_changed[1, 5] and not (mu_changed & ~changed).any()
    env.close()
