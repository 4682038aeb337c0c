"""Measurement of the building-aware classical RVO velocity (rvo3d_rvo_vel_city) next to rvo3d_rvo_vel: 64 drones x 4096
envs, 50 buildings per env (per-env sets), synthetic_patrols(seed 3) attached, on the state 20 auto-resetting steps left;
device events round --calls back-to-back calls behind 30 warm-up calls, the variants alternating in one process, three
rounds.  One JSON line (profiles/rvo_city/measurements.txt).
usage: python tools/bench_rvo_city.py [--envs 4096 --drones 64 --buildings 50 --calls 100 --acceler 0.5]"""
import argparse, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd"))
from rvo3d_amd import BatchedDroneEnv, synthetic_actions, synthetic_patrols, synthetic_world

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--drones", type=int, default=64)
ap.add_argument("--buildings", type=int, default=50)
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--acceler", type=float, default=0.5)
args = ap.parse_args()
E, N = args.envs, args.drones

world = synthetic_world(E, N, (100.0, 100.0, 10.0), nb=args.buildings, per_env_buildings=True)
env = BatchedDroneEnv(world, neighbors_num=10, action_decimals=2)
motion = synthetic_patrols(world, seed=3, speed=(0.3, 1.5), span=6.0)
env.attach_building_motion(motion)
env.observe()
for t in range(20):
    env.step(torch.from_numpy(synthetic_actions(E, N, t).astype(np.float32)).cuda(), autoreset=True)
kw = dict(vmax=(2.0, 2.0, 2.0), acceler=args.acceler)


def span(fn):
    for _ in range(30):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1e3 / args.calls, 2)


def without_motion(fn):
    def run():
        m, env._motion = env._motion, None   # (the records stay where they are: motion == NULL)
        try:
            fn()
        finally:
            env._motion = m
    return run


variants = {
    "rvo_vel_us": lambda: env.rvo_vel(**kw),
    "city_nothing_in_reach_us": lambda: env.rvo_vel_city(reach=1e-300, **kw),
    "city_us": lambda: env.rvo_vel_city(**kw),
    "city_no_motion_us": without_motion(lambda: env.rvo_vel_city(**kw)),
}
res = {"envs": E, "drones": N, "buildings": args.buildings, "acceler": args.acceler, "calls": args.calls}
res.update({k: [] for k in variants})
for _ in range(3):
    for k, fn in variants.items():
        res[k].append(span(fn))
_, d = env.rvo_vel_city(diagnostics=True, **kw)
tier = d["tier"].cpu().numpy().reshape(-1)
res["mean_n_gated"] = round(float(d["n_gated"].double().mean()), 3)
res["tier_share"] = {str(t): round(float((tier == t).mean()), 4) for t in (1, 2, 3, 4)}
res["envs_with_a_tier3_drone"] = round(float((d["tier"] == 3).any(dim=1).double().mean()), 4)
print(json.dumps(res), flush=True)
env.close()
