"""ORCA flown through the step on the device: env.orca_vel -> env.velocity_command -> env.step on the circle swap
tests/golden/rvo_orca_swap_scene.npz (tests/test_orca_host.py flies the same scene on the CPU, env by env), and
post_train.policy_test(policy_type="orca", command="velocity") in the host loop and in the fused loop; command="raw" is
what the evaluator did before."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from rvo3d_amd import BatchedDroneEnv, World
from rvo3d_amd.policy.post_train import post_train

pytestmark = pytest.mark.gpu
EPISODES = 3
KW = ("time_horizon", "time_step", "max_speed", "pref_speed", "neighbor_dist", "max_neighbors", "max_buildings", "reach",
      "below", "clear_xy")


def load():
    sc = np.load(os.path.join(ROOT, "tests", "golden", "rvo_orca_swap_scene.npz"))
    assert sc["waypoints"].shape[0] == 3   # E = 3
    rvo = {k: (int(sc[k]) if k in ("max_neighbors", "max_buildings") else float(sc[k])) for k in KW}
    world = World(sc["waypoints"], sc["n_points"], sc["map_size"], np.zeros((0, 4)))
    env = BatchedDroneEnv(world, neighbors_num=int(sc["nm"]), radius=float(sc["radius"]))
    return sc, env, rvo


def fly(controller):
    """The three envs of the scene until every one has ended (a drone done, or all finished) or `steps` are flown; an env
    that ended is no longer looked at.  -> (least separation per env over its steps, commands clipped, envs finished)."""
    sc, env, rvo = load()
    E = env.E
    env.reset()
    env.set_state(yaw=sc["yaw"])
    worst = np.full(E, np.inf)
    clipped, running, finished = 0, np.ones(E, bool), np.zeros(E, bool)
    for _ in range(int(sc["steps"])):
        w = env.orca_vel(**rvo) if controller == "orca" else env.des_vel()
        a, bits = env.velocity_command(w, return_clipped=True)
        clipped += int((bits.cpu().numpy()[running] != 0).sum())
        _, _, _, done, _, fin = env.step(a)
        sep = env.safety(0.5)[0].min(dim=1).values.cpu().numpy()
        worst[running] = np.minimum(worst[running], sep[running])
        fin_e = fin.bool().all(dim=1).cpu().numpy()
        finished |= running & fin_e
        running &= ~(done.bool().any(dim=1).cpu().numpy() | fin_e)
        if not running.any():
            break
    env.close()
    return worst, clipped, finished


def test_orca_never_touches_where_des_vel_does():
    o_worst, o_clipped, o_fin = fly("orca")
    d_worst, _, _ = fly("des")
    print("orca: sep", o_worst, "clipped", o_clipped, "finished", o_fin, "des_vel: sep", d_worst)
    assert (o_worst > 0.0).all() and o_clipped == 0 and o_fin.all()
    assert (d_worst <= 0.0).all()


def run(policy_type, fused, command, **rvo_kw):
    sc, env, rvo = load()
    pt = post_train(env, num_episodes=EPISODES, max_ep_len=int(sc["steps"]), fused=fused, safety=True,
                    rvo=rvo if policy_type == "orca" else rvo_kw, command=command, poll_every=1, inf_print=False)
    result = pt.policy_test(policy_type=policy_type)
    rec = pt.records if fused else pt.safety_records
    rec = {k: np.asarray(rec[k]).reshape(-1) for k in ("rec_min_sep", "rec_min_bclear", "rec_min_wall", "rec_near")}
    env.close()
    return result, rec


def test_policy_type_orca_in_both_loops():
    r_host, s_host = run("orca", False, "velocity")
    r_fused, s_fused = run("orca", True, "velocity")
    print(r_host, s_host)
    assert r_host == r_fused and r_host["episodes"] == EPISODES, (r_host, r_fused)
    for k in s_host:
        assert np.array_equal(np.sort(s_host[k]), np.sort(s_fused[k])), (k, s_host[k], s_fused[k])
    assert np.isfinite(s_host["rec_min_sep"]).all()


def test_command_raw_is_what_the_evaluator_did():
    """command="raw" (the default) with policy_type "rvo": the records of a loop that hands _fly()'s velocity to env.step
    as it is, flown here by hand with the evaluator's episode rules."""
    r_raw, s_raw = run("rvo", False, "raw", acceler=0.5)
    sc, env, _ = load()
    assert post_train(env, inf_print=False).command == "raw"
    with pytest.raises(ValueError):
        post_train(env, command="velocities")
    E, steps = env.E, int(sc["steps"])
    env.reset()
    env.observe()
    ep_len, lens, seps, run_sep = np.zeros(E, int), [], [], np.full(E, np.inf)
    counted = np.zeros(E, int)
    while len(lens) < EPISODES:
        _, _, _, done, info, fin = env.step(env.rvo_vel(acceler=0.5))
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
    print(r_raw, s_raw["rec_min_sep"], lens, seps)
    assert r_raw["episodes"] == EPISODES
    assert np.array_equal(np.asarray(seps), s_raw["rec_min_sep"])
