"""Secondary measurement: what the nearest-building rows cost at 64 drones x 4096 envs with 50 buildings per env
(per-env sets), k = 4, nm = 10.

  rows:   microseconds per rvo3d_building_rows, stand-alone (BatchedDroneEnv.building_rows) and in widen mode (the launch
          BuildingObsEnv adds to every step), on the state some auto-resetting steps left; device events around `--calls`
          back-to-back calls.  Widen mode moves at least 4 * W + 4 * (W + 6k) bytes per drone (the dense row in, the wide
          row out: 408 + 504 at nm = 10, k = 4); the line reports the time against that traffic.
  step:   microseconds per auto-resetting step of the plain env and of BuildingObsEnv (dense step + widen launch), the same
          actions, likewise.

  --moving: the rows of eight floats for moving buildings (rvo3d_building_rows_moving) next to the rows of six on the same
          state in the same run: synthetic_patrols is attached to the plain env and advanced a few times, then both launches
          are timed stand-alone and in widen mode (the rows of eight with the motion and, in widen mode, without one).  The
          step variants are left out (the motion would add its own launch to them).  Widen mode at rows of eight moves at
          least 4 * W + 4 * (W + 8k) bytes per drone plus, per kept row, a record (32 B) and its speed, leg and one endpoint
          (8 + 1 + 16 B).

The variants alternate in one process, `--rounds` times, so the run-to-run spread shows next to the differences.  One JSON
line per run, then a summary line."""
import argparse, ctypes as C, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd"))
from rvo3d_amd import BatchedDroneEnv, BuildingObsEnv, _lib, synthetic_actions, synthetic_patrols, synthetic_world

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--drones", type=int, default=64)
ap.add_argument("--buildings", type=int, default=50)
ap.add_argument("-k", type=int, default=4)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--moving", action="store_true")
args = ap.parse_args()
E, N, K = args.envs, args.drones, args.k
world = synthetic_world(E, N, (50, 50, 10), nb=args.buildings, per_env_buildings=True)
acts = [torch.from_numpy(synthetic_actions(E, N, t).astype(np.float32)).cuda() for t in range(16)]


def timed(fn):
    for i in range(args.warmup):
        fn(i)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(args.calls):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / args.calls * 1e3


plain, wide_env = BatchedDroneEnv(world), BuildingObsEnv(world, building_rows=K)
for env in (plain, wide_env):
    env.observe()
    for t in range(20):   # spread the drones: the state of a rollout, not the reset state
        env.step(acts[t % 16], autoreset=True)
W = plain.W
wide = torch.zeros((E, N, W + 6 * K), device="cuda")
wargs = _lib.BuildingRowsArgs(K, 5.0, 2.0, wide.data_ptr(), W + 6 * K, 12, None, plain.obs.data_ptr())
variants = {
    "rows_standalone_us": lambda i: plain.building_rows(K),
    "rows_widen_us": lambda i: _lib.check(_lib.lib().rvo3d_building_rows(plain._h, C.byref(wargs), plain._stream()),
                                          "rvo3d_building_rows"),
    "step_plain_us": lambda i: plain.step(acts[i % 16], autoreset=True),
    "step_building_obs_us": lambda i: wide_env.step(acts[i % 16], autoreset=True),
}
if args.moving:
    motion = synthetic_patrols(world, seed=3, speed=(0.3, 1.5), span=6.0)
    plain.attach_building_motion(motion)
    for t in range(5):
        motion.advance()
    wide8 = torch.zeros((E, N, W + 8 * K), device="cuda")
    wargs8 = _lib.BuildingRowsArgs(K, 5.0, 2.0, wide8.data_ptr(), W + 8 * K, 12, None, plain.obs.data_ptr())
    moving = lambda m: _lib.check(_lib.lib().rvo3d_building_rows_moving(plain._h, C.byref(wargs8), m, motion.dt,
                                                                        plain._stream()), "rvo3d_building_rows_moving")
    variants = {
        "rows6_standalone_us": variants["rows_standalone_us"],
        "rows8_standalone_us": lambda i: plain.building_rows(K, velocity=True),
        "rows6_widen_us": variants["rows_widen_us"],
        "rows8_widen_us": lambda i: moving(C.byref(motion._args)),
        "rows8_widen_no_motion_us": lambda i: moving(None),
    }
    if (8 * K) % 6 == 0 and 8 * K // 6 <= 8:   # rows of six at the k that gives the same output width (k = 3: 4 x 6 = 3 x 8)
        k6 = 8 * K // 6
        wargs_same = _lib.BuildingRowsArgs(k6, 5.0, 2.0, wide8.data_ptr(), W + 6 * k6, 12, None, plain.obs.data_ptr())
        variants["rows6_widen_same_width_us"] = lambda i: _lib.check(
            _lib.lib().rvo3d_building_rows(plain._h, C.byref(wargs_same), plain._stream()), "rvo3d_building_rows")
out = {"envs": E, "drones": N, "buildings": args.buildings, "k": K, "obs_width": W + 6 * K}
out.update({name: [] for name in variants})
for r in range(args.rounds):
    for name, fn in variants.items():
        us = timed(fn)
        out[name].append(round(us, 2))
        print(json.dumps({"variant": name, "round": r, "us": round(us, 2)}), flush=True)
rows, cnt = plain.building_rows(K)
out["mean_rows_per_drone"] = round(float(cnt.float().mean()), 3)
traffic = E * N * (4 * W + 4 * (W + 6 * K))
out["widen_traffic_MB"] = round(traffic / 1e6, 1)
out["widen_GB_per_s"] = round(traffic / (min(out["rows6_widen_us" if args.moving else "rows_widen_us"]) * 1e-6) / 1e9, 1)
if args.moving:
    out["obs_width_rows8"] = W + 8 * K
    rows8, _ = plain.building_rows(K, velocity=True)
    out["rows8_with_velocity"] = round(float((rows8[..., 6:] != 0).any(-1).float().sum() / max(1, int(cnt.sum()))), 3)
    traffic8 = E * N * (4 * W + 4 * (W + 8 * K))
    out["widen8_traffic_MB"] = round(traffic8 / 1e6, 1)
    out["widen8_GB_per_s"] = round(traffic8 / (min(out["rows8_widen_us"]) * 1e-6) / 1e9, 1)
print(json.dumps(out))
