"""What per-env drone counts cost: kernel time (HIP events on the launch stream, the method of tools/bench_aux.py) of
the fused auto-reset step on three handles over the same world and action stream, alternating - (a) no counts: the plain
kernel, (b) counts attached, every env full: the counted kernel doing the plain kernel's work, (c) counts from
(64, 33, 48, 1, 63, 2) cycled over the envs (scaled to the handle's num_drones) - at the headline shape, 64 drones x 4096
envs on the benchmark's map, and at 256 x 1024.  Prints one JSON line per shape with ms_per_step of the three, the runs,
and the kernels' names.
usage: python tools/bench_env_counts.py [--shapes 64x4096 256x1024 --reps 100 --rounds 5]"""
import argparse, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd"))
from rvo3d_amd import BatchedDroneEnv, synthetic_actions, synthetic_world

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["64x4096", "256x1024"], help="drones x envs")
ap.add_argument("--map", type=float, nargs=3, default=(50.0, 50.0, 10.0))
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=100)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_env_counts needs a GPU")
CYCLE = (64, 33, 48, 1, 63, 2)


def timed(env, acts):
    """mean step time in ms over args.reps steps (without host-stall samples, as tools/bench_aux.py)"""
    for t in range(5):
        env.step(acts[t % 16], autoreset=True)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for i, (a, b) in enumerate(ev):
        a.record(); env.step(acts[i % 16], autoreset=True); b.record()
    torch.cuda.synchronize()
    ts = np.asarray([a.elapsed_time(b) for a, b in ev])
    return float(ts[ts <= 3 * np.median(ts)].mean())


for shape in args.shapes:
    N, E = (int(x) for x in shape.split("x"))
    world = synthetic_world(E, N, tuple(args.map))
    mixed = np.array([max(1, CYCLE[e % len(CYCLE)] * N // 64) for e in range(E)], dtype=np.int32)
    counts = {"none": None, "full": np.full(E, N, np.int32), "mixed": mixed}
    envs = {k: BatchedDroneEnv(world if c is None else world.with_drone_counts(c), neighbors_num=10, action_decimals=2)
            for k, c in counts.items()}
    acts = [torch.from_numpy(synthetic_actions(E, N, t).astype(np.float32)).cuda() for t in range(16)]
    for env in envs.values():
        env.observe()
        for t in range(args.warmup):
            env.step(acts[t % 16], autoreset=True)
    runs = {k: [] for k in envs}
    for _ in range(args.rounds):  # alternating: the three see the same machine
        for k, env in envs.items():
            runs[k].append(timed(env, acts))
    med = {k: float(np.median(v)) for k, v in runs.items()}
    print(json.dumps({"drones": N, "envs": E, "map": list(args.map), "reps": args.reps, "rounds": args.rounds,
                      "ms_per_step": {k: round(v, 5) for k, v in med.items()},
                      "full_over_none": round(med["full"] / med["none"], 4),
                      "mixed_over_none": round(med["mixed"] / med["none"], 4),
                      "live_fraction_mixed": round(float(mixed.sum()) / (E * N), 4),
                      "runs_ms": {k: [round(x, 5) for x in v] for k, v in runs.items()},
                      "kernel": {k: env.kernel_name() for k, env in envs.items()},
                      "launch": {k: env.launch_info() for k, env in envs.items()}}), flush=True)
    for env in envs.values():
        env.close()
