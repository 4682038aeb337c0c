"""Secondary measurement: kernel time (HIP events on the launch stream) of the entry points next to
the fused step at the benchmark shape - observe, plain step, step_policy (trainer glue fused in),
reset + observe, des_vel, the classical RVO velocity selection.
Last: moving buildings (move_buildings(): the launch, the host path for the same job, the env step of that world).
usage: python tools/bench_aux.py [--envs 4096 --drones 64] [--only move_buildings]"""
import argparse, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd"))
from rvo3d_amd import BatchedDroneEnv, synthetic_actions, synthetic_world

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--drones", type=int, default=64)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--only", default=None, help="move_buildings: that entry alone")
args = ap.parse_args()
E, N = args.envs, args.drones


def move_buildings():
    """Moving buildings (rvo3d_move_env_buildings) with 50 buildings per env on a 100 x 100 map: the launch, next to the
    only thing the host path offers for the same job - one set_env_buildings call with the same sets (host staging,
    hipMalloc, copies, a synchronisation: wall time) - and next to the env step of that configuration."""
    import time
    from rvo3d_amd import synthetic_patrols
    world = synthetic_world(E, N, (100.0, 100.0, 10.0), nb=50, per_env_buildings=True)
    env = BatchedDroneEnv(world, neighbors_num=10, action_decimals=2)
    acts = [torch.from_numpy(synthetic_actions(E, N, t).astype(np.float32)).cuda() for t in range(16)]
    env.observe()
    for t in range(200):
        env.step(acts[t % 16], autoreset=True)
    step = timed("move_buildings: env step, static buildings", lambda i: env.step(acts[i % 16], autoreset=True))
    motion = synthetic_patrols(world, seed=1, speed=(0.3, 1.5), span=6.0)
    env.attach_building_motion(motion)
    move = timed("move_buildings: the launch (50 per env)", lambda i: motion.advance(), per_drone=False)
    both = timed("move_buildings: launch + env step", lambda i: env.step(acts[i % 16], autoreset=True))
    env.attach_building_motion(None)
    b, c = world.buildings, world.building_counts
    env.set_env_buildings(b, c)
    torch.cuda.synchronize()
    ts = []
    for _ in range(10):
        t0 = time.perf_counter()
        env.set_env_buildings(b, c)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    host = float(np.median(ts)) * 1e6
    print("%-44s %8.1f us  (wall time, median of 10)" % ("move_buildings: one set_env_buildings call", host), flush=True)
    print("move_buildings summary: launch %.1f us, host path %.1f us (%.0fx), env step %.1f us, launch + step %.1f us" % (
        move, host, host / move, step, both), flush=True)
    env.close()


def timed(name, fn, bytes_per_drone=None, per_drone=True):
    for _ in range(5):
        fn(0)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for i, (a, b) in enumerate(ev):
        a.record(); fn(i); b.record()
    torch.cuda.synchronize()
    ts = np.asarray([a.elapsed_time(b) for a, b in ev])
    us = float(ts[ts <= 3 * np.median(ts)].mean()) * 1e3  # (without host-stall samples, see bench.py)
    extra = "" if bytes_per_drone is None else "  %.0f GB/s of its %d algorithmic bytes per drone" % (E * N * bytes_per_drone / us / 1e3, bytes_per_drone)
    rate = "  %.3e drones/s%s" % (E * N / (us * 1e-6), extra) if per_drone else ""  # (no per-drone rate for a T-step scan)
    print("%-44s %8.1f us%s" % (name, us, rate), flush=True)
    return us


if args.only == "move_buildings":
    move_buildings()
    sys.exit(0)

env = BatchedDroneEnv(synthetic_world(E, N, (50.0, 50.0, 10.0)), neighbors_num=10, action_decimals=2)
acts = [torch.from_numpy(synthetic_actions(E, N, t).astype(np.float32)).cuda() for t in range(16)]
env.observe()
for t in range(600):
    env.step(acts[t % 16], autoreset=True)

W = env.W
timed("step + auto-reset (fused, f32 actions)", lambda i: env.step(acts[i % 16], autoreset=True), 719)
timed("step_policy + auto-reset (trainer glue)", lambda i: env.step_policy(acts[i % 16], autoreset=True), 719)
timed("observe (env_observation, action 0)", lambda i: env.observe(), 64 + 4 * W + 4 + 24)
# nearest-building rows (rvo3d_building_rows, k = 4) on this world's state: stand-alone - 6 state doubles in, 24 floats
# and a count out - and widen mode - the dense row in, the wide row out.  (This world has no buildings: the traffic
# alone; tools/bench_building_rows.py times both with 50 buildings per env.)
import ctypes as C
from rvo3d_amd import _lib
wide = torch.zeros((E, N, W + 24), device="cuda")
wargs = _lib.BuildingRowsArgs(4, 5.0, 2.0, wide.data_ptr(), W + 24, 12, None, env.obs.data_ptr())
timed("building_rows, stand-alone (k = 4)", lambda i: env.building_rows(4), 48 + 96 + 4)
timed("building_rows, widen mode (k = 4)", lambda i: _lib.check(_lib.lib().rvo3d_building_rows(
    env._h, C.byref(wargs), env._stream()), "rvo3d_building_rows"), 4 * W + 4 * (W + 24))


def manual(i):  # the reference's protocol without the fused auto-reset: step, reset the ended drones, observe again
    _, _, _, done, _, fin = env.step(acts[i % 16])
    env.reset_drones(done | fin)
    env.observe()


timed("plain step + reset_drones(done | finish) + observe", manual)
mask = torch.zeros((E, N), dtype=torch.uint8, device="cuda"); mask[:, ::7] = 1
timed("reset_drones (1/7 of the drones) + observe", lambda i: (env.reset_drones(mask), env.observe()))
timed("des_vel (cal_des_list)", lambda i: env.des_vel(), 48 + 24)
timed("rvo_vel (classical RVO velocity selection)", lambda i: env.rvo_vel(vmax=(2.0, 2.0, 2.0), acceler=0.5))
timed("rvo_vel_city (this world has no buildings)", lambda i: env.rvo_vel_city(vmax=(2.0, 2.0, 2.0), acceler=0.5))
timed("orca_vel (this world has no buildings)", lambda i: env.orca_vel())
want = env.des_vel()
timed("velocity_command (velocity -> action)", lambda i: env.velocity_command(want), 64 + 24 + 24)
flags = env.error_flags()
print("device error word", flags)

# GAE of a finished [T, E, N] rollout: the default scan (gae_scan, ~30 float64 tensor ops) and the one-launch kernel
# (gae_device -> rvo3d_gae), on random data with cuts at density 0.05; GB/s over the kernel's algorithmic bytes (one
# read of rew and val, one write of adv and ret, the cut bytes); transient memory = peak allocation above the inputs (adv and ret included)
from rvo3d_amd.policy import gae_device, gae_scan
for T in (16, 128):
    g = torch.Generator(device="cuda").manual_seed(T)
    rew = torch.randn((T, E, N), device="cuda", generator=g) * 3
    val = torch.randn((T, E, N), device="cuda", generator=g) * 2
    cut = torch.rand((T, E), device="cuda", generator=g) < 0.05
    cut3 = cut.unsqueeze(-1).expand_as(rew)  # (as RolloutBuffer.get() passes it)
    nbytes = 16 * T * E * N + T * E
    for name, fn in (("gae_scan", lambda i: gae_scan(rew, val, cut3, 0.99, 0.97)),
                     ("gae_device", lambda i: gae_device(rew, val, cut, 0.99, 0.97))):
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        us = timed("%s T = %d" % (name, T), fn, per_drone=False)
        print("    %-40s %8.1f GB/s of its %d algorithmic bytes; transient memory %.1f MB" % (
            "", nbytes / us / 1e3, nbytes, (torch.cuda.max_memory_allocated() - base) / 1e6), flush=True)
    del rew, val, cut, cut3

env.close()
move_buildings()
