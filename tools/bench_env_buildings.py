"""What per-env building sets cost over the shared list: kernel time (HIP events on the launch stream, the method of
tools/bench_aux.py) of the fused auto-reset step at config 5's shape - 256 drones x 1024 envs, map 100 x 100 x 10,
50 buildings, nm = 10 - once with synthetic_world's shared list and once with a set per env
(synthetic_world(per_env_buildings=True): E private record arrays and grids instead of one cache-resident copy),
on the same action stream, the two handles alternating.  Prints one JSON line: both times, the ratio, the bytes of the
per-env grids and records.
usage: python tools/bench_env_buildings.py [--envs 1024 --drones 256 --buildings 50 --reps 100 --rounds 5]"""
import argparse, json, math, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd"))
from rvo3d_amd import BatchedDroneEnv, synthetic_actions, synthetic_world

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--drones", type=int, default=256)
ap.add_argument("--buildings", type=int, default=50)
ap.add_argument("--map", type=float, nargs=3, default=(100.0, 100.0, 10.0))
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=200)
args = ap.parse_args()
E, N, nb, MAP = args.envs, args.drones, args.buildings, tuple(args.map)
if not torch.cuda.is_available():
    sys.exit("bench_env_buildings needs a GPU")

envs = {k: BatchedDroneEnv(synthetic_world(E, N, MAP, nb=nb, per_env_buildings=(k == "per_env")), neighbors_num=10,
                           action_decimals=2) for k in ("shared", "per_env")}
acts = [torch.from_numpy(synthetic_actions(E, N, t).astype(np.float32)).cuda() for t in range(16)]
for env in envs.values():
    env.observe()
    for t in range(args.warmup):
        env.step(acts[t % 16], autoreset=True)


def timed(env):
    """mean step time in us over args.reps steps (without host-stall samples, as tools/bench_aux.py)"""
    for t in range(5):
        env.step(acts[t % 16], autoreset=True)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for i, (a, b) in enumerate(ev):
        a.record(); env.step(acts[i % 16], autoreset=True); b.record()
    torch.cuda.synchronize()
    ts = np.asarray([a.elapsed_time(b) for a, b in ev])
    return float(ts[ts <= 3 * np.median(ts)].mean()) * 1e3


runs = {k: [] for k in envs}
for _ in range(args.rounds):  # alternating: both see the same machine
    for k, env in envs.items():
        runs[k].append(timed(env))
# the per-env grid as the library lays it out: ~8 m cells, at most 64 x 64, 32 B per cell (64 MiB for all envs together
# at the most; this shape is far below)
cs = max(8.0, max(MAP[0], MAP[1]) / 64.0)
cells = math.ceil(MAP[0] / cs) * math.ceil(MAP[1] / cs)
assert E * cells * 32 <= 64 << 20, "beyond the budget the library grows the cells: this restatement does not apply"
med = {k: float(np.median(v)) for k, v in runs.items()}
print(json.dumps({"drones": N, "envs": E, "buildings": nb, "map": MAP, "reps": args.reps, "rounds": args.rounds,
                  "shared_us": round(med["shared"], 2), "per_env_us": round(med["per_env"], 2),
                  "per_env_over_shared": round(med["per_env"] / med["shared"], 4),
                  "shared_runs_us": [round(x, 2) for x in runs["shared"]],
                  "per_env_runs_us": [round(x, 2) for x in runs["per_env"]],
                  "grid_bytes": E * cells * 32, "record_bytes": E * nb * 32,
                  "done_rate": {k: round(float(env.done.float().mean()), 4) for k, env in envs.items()}}))
