"""Time one route re-draw on the device (RouteSampler.redraw: rvo3d_sample_routes + rvo3d_set_routes, HIP events, median
of --reps) next to the host path it replaces (synthetic_world + a new BatchedDroneEnv, wall time).  Prints one JSON line.
--city adds the re-draw round buildings (CityRoutePlanner.redraw: rvo3d_sample_routes_city + rvo3d_plan_routes +
rvo3d_set_routes) in a second env with --buildings buildings per env and --points waypoint rows, and `plan` alone.

    python tools/bench_routes.py --drones 64 --envs 4096
    python tools/bench_routes.py --drones 64 --envs 4096 --city
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

from rvo3d_amd import BatchedDroneEnv, CityRoutePlanner, RouteSampler, World, synthetic_world  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--drones", type=int, default=64)
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--map", type=float, nargs=3, default=(50.0, 50.0, 10.0))
ap.add_argument("--min-sep", type=float, default=1.0)
ap.add_argument("--min-len", type=float, default=10.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--city", action="store_true", help="also time the re-draw round per-env buildings")
ap.add_argument("--buildings", type=int, default=50)
ap.add_argument("--points", type=int, default=8)
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
out = dict(drones=N, envs=E, map=list(args.map), min_sep=args.min_sep, min_len=args.min_len, reps=args.reps,
           redraw_ms=dict(zip(("median", "min", "max"), (round(x, 4) for x in redraw))),
           sample_ms=round(sample[0], 4), set_routes_ms=round(set_routes[0], 4), unplaced_last_draw=unplaced,
           host_path_s=dict(synthetic_world=round(t_world, 3), new_env=round(t_env, 3), total=round(t_world + t_env, 3)))
env.close()

if args.city:
    cities = synthetic_world(E, 1, args.map, nb=args.buildings, per_env_buildings=True)  # (only its buildings are used)
    cenv = BatchedDroneEnv(World(world.waypoints, world.n_points, world.map_size, cities.buildings).with_max_points(args.points))
    planner = CityRoutePlanner(sampler)
    cenv.observe()
    planner.redraw(cenv, 0)  # allocates the staging tensors, uploads the city
    torch.cuda.synchronize()
    city_redraw = timed(lambda i: planner.redraw(cenv, i))
    wp, npts, unp, blocked, bmask = planner._bufs[(cenv.E, cenv.N, cenv.P, str(cenv.device))]
    bld, cnt = cenv.device_buildings()
    city_sample = timed(lambda i: planner.sample(E, N, cenv.P, i, cenv.device, bld, cnt, out=(wp, npts, unp)))
    start_goal = wp.clone()

    def plan(i):  # (in place: every repetition plans the same start / goal pairs)
        wp.copy_(start_goal)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        planner.plan(wp, bld, cnt, out=(npts, blocked, bmask))
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    plan_ms = sorted(plan(i) for i in range(args.reps))
    city_set = timed(lambda i: cenv.set_routes(wp, npts))
    assert cenv.error_flags() & 4 == 0
    out["city"] = dict(buildings=args.buildings, points=args.points,
                       redraw_ms=dict(zip(("median", "min", "max"), (round(x, 4) for x in city_redraw))),
                       sample_ms=round(city_sample[0], 4), plan_ms=round(statistics.median(plan_ms), 4),
                       plan_ms_min_max=[round(plan_ms[0], 4), round(plan_ms[-1], 4)], set_routes_ms=round(city_set[0], 4),
                       unplaced_last_draw=int(unp.sum()), blocked_last_draw=int(blocked.sum()),
                       detours_last_draw=int((npts > 2).sum()))
    cenv.close()
print(json.dumps(out))
