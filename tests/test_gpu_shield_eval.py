"""The action shield in evaluation: post_train(..., shield=dict(...)) on the circle swap tests/golden/rvo_orca_swap_scene.npz
(tests/test_shield_host.py flies the same scene on the CPU, env by env, from the scene's own start yaw), in the host loop
and in the fused loop, with poll_every=1 so that both fly the same steps.

The shield's parameters are the scene's ORCA parameters with one change.  The evaluator resets every drone to yaw 0 and
speed 0, where the CPU flights start with the yaw of the route; from that heading the first commands of the controller
clip (a turn is at most 90 degrees a step).  The horizon is therefore not the scene's 5 s but neighbor_dist / max_speed =
10 s: the time a drone at full speed needs to cross the range it sees neighbours in, the longest horizon at which a
neighbour in range can matter.  Flown on the CPU from yaw 0 (the restatement through the oracle's step): least separations
0.055, 0.020 and 0.011 m, no fallback row, every drone finished, for every horizon from 7.5 s up (the cut-off no longer
binds); with the scene's 5 s env 1 touches by 5.6 mm after 4 fallback rows - the limit "commands that clip" of the
documents.  On the MI355X: least separation 0.011173 m, three successes of 17 steps, 62 % of 195 judged rows intervened, no
fallback row and no clipped command, in both loops; unshielded the drones overlap by 0.3955 m."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from rvo3d_amd import BatchedDroneEnv, World
from rvo3d_amd.policy import mlp_ac
from rvo3d_amd.policy.post_train import post_train

pytestmark = pytest.mark.gpu
EPISODES = 3
KW = ("time_horizon", "time_step", "max_speed", "neighbor_dist", "max_neighbors", "max_buildings", "reach", "below", "clear_xy")
REC = ("rec_min_sep", "rec_min_bclear", "rec_min_wall", "rec_near")


def load(envs=None):
    sc = np.load(os.path.join(ROOT, "tests", "golden", "rvo_orca_swap_scene.npz"))
    assert sc["waypoints"].shape[:2] == (3, 4)
    shield = {k: (int(sc[k]) if k in ("max_neighbors", "max_buildings") else float(sc[k])) for k in KW}
    assert shield["max_speed"] == 1.0
    shield["time_horizon"] = shield["neighbor_dist"] / shield["max_speed"]   # (module docstring)
    e = slice(None) if envs is None else slice(0, envs)
    world = World(sc["waypoints"][e], sc["n_points"][e], sc["map_size"], np.zeros((0, 4)))
    env = BatchedDroneEnv(world, neighbors_num=int(sc["nm"]), radius=float(sc["radius"]))
    return sc, env, shield


def run(fused, shield, policy_type="des", envs=None, episodes=EPISODES, policy=None, **kw):
    sc, env, par = load(envs)
    pt = post_train(env, num_episodes=episodes, max_ep_len=int(sc["steps"]), fused=fused, safety=True, command="velocity",
                    shield=par if shield else None, poll_every=1, inf_print=False, **kw)
    result = pt.policy_test(policy_type=policy_type, policy=policy)
    rec = pt.records if fused else pt.safety_records
    rec = {k: np.asarray(rec[k]).reshape(-1) for k in REC}
    env.close()
    return result, rec, pt


def same_records(a, b):
    """Two loops' results: every entry equal; the per-episode mean speed to 1e-13 relative - the host loop sums torch's
    vector_norm(...).mean() per step, the fused loop rvo3d_eval_account's own sums, at most 80 steps of one rounding each
    (80 * 2^-53 = 9e-15), with and without a shield - and the safety records equal."""
    for k in a[0]:
        if k == "speed":
            assert np.allclose(a[0][k], b[0][k], rtol=1e-13, atol=0.0), (a[0][k], b[0][k])
        else:
            assert a[0][k] == b[0][k], (k, a[0][k], b[0][k])
    for k in REC:
        assert np.array_equal(np.sort(a[1][k]), np.sort(b[1][k])), (k, a[1][k], b[1][k])


def test_shielded_des_vel_succeeds_where_des_vel_collides():
    """policy_type "des" through velocity commands and the shield: every episode a success and the least separation of the
    evaluation > 0, in both loops, record by record the same, with the same pt.shield; without the shield they collide."""
    host, fused = run(False, True), run(True, True)
    plain = run(True, False)
    print("shielded:", host[0], host[2].safety, host[2].shield, "\nunshielded:", plain[0], plain[2].safety)
    same_records(host, fused)
    assert host[2].shield == fused[2].shield
    for r, _, pt in (host, fused):
        assert r["episodes"] == EPISODES and r["success_rate"] == 1.0
        assert pt.safety["min_min_sep"] > 0.0
        s = pt.shield
        assert set(s) == {"judged", "intervened_share", "fallback_share", "clipped_share"}
        assert s["judged"] > 0 and 0.0 < s["intervened_share"] <= 1.0 and 0.0 <= s["fallback_share"] <= 1.0
    assert plain[0]["success_rate"] == 0.0 and plain[2].safety["min_min_sep"] <= 0.0
    assert plain[2].shield is None


def test_shield_sits_behind_eval_action():
    """One "drl" run, mlp_ac through policy_kernel="mlp_x3" and the shield: the fused loop, which shields rvo3d_eval_action's
    output, equals the host loop, which shields the action it makes in torch.  E = 1: with more envs the two loops
    re-observe differently when an env ends (rvo3d_amd/policy/post_train.py)."""
    sc, env, _ = load(1)
    torch.manual_seed(5)
    ac = mlp_ac(env.W).cuda()
    env.close()
    kw = dict(policy_type="drl", envs=1, episodes=2, policy=ac, policy_kernel="mlp_x3", std_factor=0.5, seed=11)
    host, fused = run(False, True, **kw), run(True, True, **kw)
    bare = run(True, False, **kw)
    print(host[0], host[2].shield, bare[0])
    same_records(host, fused)
    assert host[2].shield == fused[2].shield and host[2].shield["judged"] > 0
    assert host[0]["episodes"] == 2


def test_shield_none_is_the_loop_as_it_was(monkeypatch):
    """shield=None: no shield call is made (env.shield_action raises here) and the records are those of the loop without the
    parameter: command="velocity" flown by hand with the evaluator's episode rules, and the fused loop's the same."""
    def refuse(self, *a, **k):
        raise AssertionError("shield_action called with shield=None")
    monkeypatch.setattr(BatchedDroneEnv, "shield_action", refuse)
    host, fused = run(False, False), run(True, False)
    same_records(host, fused)
    assert host[2].shield is None and fused[2].shield is None
    sc, env, _ = load()
    E, steps = env.E, int(sc["steps"])
    env.reset()
    env.observe()
    ep_len, lens, seps, run_sep, counted = np.zeros(E, int), [], [], np.full(E, np.inf), np.zeros(E, int)
    while len(lens) < EPISODES:
        _, _, _, done, info, fin = env.step(env.velocity_command(env.des_vel()))
        ep_len += 1
        run_sep = np.minimum(run_sep, env.safety(0.5)[0].min(dim=1).values.cpu().numpy())
        ended = done.bool().any(dim=1).cpu().numpy() | (ep_len == steps) | fin.bool().all(dim=1).cpu().numpy()
        if ended.any():
            for e in np.nonzero(ended)[0]:
                if counted[e] < 1:
                    counted[e] += 1
                    lens.append(int(ep_len[e]))
                    seps.append(run_sep[e])
            env.reset(torch.as_tensor(ended, device="cuda"))
            env.observe()
            ep_len[ended], run_sep[ended] = 0, np.inf
    env.close()
    assert np.array_equal(np.asarray(seps), host[1]["rec_min_sep"])
    with pytest.raises(ValueError):
        post_train(env, shield=dict(diagnostics=True))
