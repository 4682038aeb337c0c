"""Time one route re-draw on the device (RouteSampler.redraw: rvo3d_sample_routes + rvo3d_set_routes, HIP events, median
of --reps) next to the host path it replaces (synthetic_world + a new BatchedDroneEnv, wall time).  Prints one JSON line.

    python tools/bench_routes.py --drones 64 --envs 4096
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd"))

import torch  # noqa: E402

from rvo3d_amd import BatchedDroneEnv, RouteSampler, synthetic_world  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--drones", type=int, default=64)
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--map", type=float, nargs=3, default=(50.0, 50.0, 10.0))
ap.add_argument("--min-sep", type=float, default=1.0)
ap.add_argument("--min-len", type=float, default=10.0)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
E, N = args.envs, args.drones

t0 = time.perf_counter()
world = synthetic_world(E, N, args.map, min_sep=args.min_sep)
t_world = time.perf_counter() - t0
t0 = time.perf_counter()
env = BatchedDroneEnv(world)
torch.cuda.synchronize()
t_env = time.perf_counter() - t0

sampler = RouteSampler(args.map, min_sep=args.min_sep, min_len=args.min_len)
env.observe()
sampler.redraw(env, 0)  # allocates the staging tensors
torch.cuda.synchronize()


def timed(fn):
    ms = []
    for i in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i + 1)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


redraw = timed(lambda i: sampler.redraw(env, i))
wp, npts, unp = sampler._bufs[(env.E, env.N, env.P, str(env.device))]
sample = timed(lambda i: sampler.sample(E, N, env.P, i, env.device, out=(wp, npts, unp)))
set_routes = timed(lambda i: env.set_routes(wp, npts))
unplaced = int(unp.sum())
assert env.error_flags() & 4 == 0
print(json.dumps(dict(drones=N, envs=E, map=list(args.map), min_sep=args.min_sep, min_len=args.min_len, reps=args.reps,
                      redraw_ms=dict(zip(("median", "min", "max"), (round(x, 4) for x in redraw))),
                      sample_ms=round(sample[0], 4), set_routes_ms=round(set_routes[0], 4), unplaced_last_draw=unplaced,
                      host_path_s=dict(synthetic_world=round(t_world, 3), new_env=round(t_env, 3),
                                       total=round(t_world + t_env, 3)))))
env.close()
