"""Measurement of the ORCA velocity (rvo3d_orca_vel) and the velocity command (rvo3d_vel_command) at the shape of
tools/bench_rvo_city.py, with rvo3d_rvo_vel_city beside them for orientation: 64 drones x 4096 envs, 50 buildings per env
(per-env sets), synthetic_patrols(seed 3) attached, on the state 20 auto-resetting steps left; device events round --calls
back-to-back calls behind 30 warm-up calls, the variants alternating in one process, three rounds.  One JSON line
(profiles/orca/measurements.txt).
usage: python tools/bench_orca.py [--envs 4096 --drones 64 --buildings 50 --calls 100]"""
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
args = ap.parse_args()
E, N = args.envs, args.drones

world = synthetic_world(E, N, (100.0, 100.0, 10.0), nb=args.buildings, per_env_buildings=True)
env = BatchedDroneEnv(world, neighbors_num=10, action_decimals=2)
motion = synthetic_patrols(world, seed=3, speed=(0.3, 1.5), span=6.0)
env.attach_building_motion(motion)
env.observe()
for t in range(20):
    env.step(torch.from_numpy(synthetic_actions(E, N, t).astype(np.float32)).cuda(), autoreset=True)


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


want = env.des_vel()
variants = {
    "rvo_vel_city_us": lambda: env.rvo_vel_city(vmax=(2.0, 2.0, 2.0), acceler=0.5),
    "orca_us": lambda: env.orca_vel(),
    "orca_16_neighbours_8_buildings_us": lambda: env.orca_vel(max_neighbors=16, max_buildings=8),
    "orca_no_buildings_kept_us": lambda: env.orca_vel(max_buildings=0),
    "vel_command_us": lambda: env.velocity_command(want),
}
res = {"envs": E, "drones": N, "buildings": args.buildings, "calls": args.calls}
res.update({k: [] for k in variants})
for _ in range(3):
    for k, fn in variants.items():
        res[k].append(span(fn))
_, d = env.orca_vel(diagnostics=True)
st = d["status"].cpu().numpy().reshape(-1)
res["status_share"] = {str(s): round(float((st == s).mean()), 4) for s in (1, 2, 3)}
res["mean_n_neighbors"] = round(float(d["n_neighbors"].double().mean()), 3)
res["mean_n_buildings"] = round(float(d["n_buildings"].double().mean()), 3)
res["workspace_MB_default_args"] = round((2 * (10 + 4) - 1) * 6 * 8 * E * N / 2 ** 20, 1)
print(json.dumps(res), flush=True)
env.close()
