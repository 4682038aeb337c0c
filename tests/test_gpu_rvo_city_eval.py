"""The classical controllers in evaluation: post_train.policy_test(policy_type="rvo" / "rvo_city") on the fixture scene
tests/golden/rvo_city_scene.npz (tests/test_rvo_city_host.py flies the same scene on the CPU), with safety=True, in the
host loop and in the fused loop."""
import os

import numpy as np
import pytest

from conftest import ROOT
from rvo3d_amd import BatchedDroneEnv, World
from rvo3d_amd.policy.post_train import post_train

pytestmark = pytest.mark.gpu
EPISODES = 2


def run(policy_type, fused):
    """(result, safety records [episodes] each) of EPISODES episodes of the fixture scene."""
    sc = np.load(os.path.join(ROOT, "tests", "golden", "rvo_city_scene.npz"))
    world = World(sc["waypoints"], sc["n_points"], sc["map_size"], sc["buildings"])
    env = BatchedDroneEnv(world, neighbors_num=int(sc["nm"]), radius=float(sc["radius"]))
    rvo = dict(acceler=float(sc["acceler"]))
    if policy_type == "rvo_city":
        rvo.update(horizon=float(sc["horizon"]), clear_xy=float(sc["clear_xy"]), clear_z=float(sc["clear_z"]))
    pt = post_train(env, num_episodes=EPISODES, max_ep_len=int(sc["steps"]), fused=fused, safety=True, rvo=rvo,
                    poll_every=1, inf_print=False)
    result = pt.policy_test(policy_type=policy_type)
    rec = pt.records if fused else pt.safety_records
    rec = {k: np.asarray(rec[k]).reshape(-1) for k in ("rec_min_sep", "rec_min_bclear", "rec_min_wall", "rec_near")}
    env.close()
    return result, rec


@pytest.mark.parametrize("fused", [False, True], ids=["host_loop", "fused_loop"])
def test_rvo_city_keeps_clear_where_des_vel_flies_into_a_building(fused):
    _, city = run("rvo_city", fused)
    _, des = run("des", fused)
    print("rvo_city", city["rec_min_bclear"], "des", des["rec_min_bclear"])
    assert len(city["rec_min_bclear"]) == EPISODES and (city["rec_min_bclear"] > 0.0).all()
    assert (des["rec_min_bclear"] <= 0.0).all()


@pytest.mark.parametrize("policy_type", ["rvo", "rvo_city"])
def test_both_loops_agree(policy_type):
    r_host, s_host = run(policy_type, False)
    r_fused, s_fused = run(policy_type, True)
    assert r_host == r_fused and r_host["episodes"] == EPISODES, (r_host, r_fused)
    for k in s_host:
        assert np.array_equal(s_host[k], s_fused[k]), (k, s_host[k], s_fused[k])
