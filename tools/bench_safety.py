"""Secondary measurement: what the safety metrics cost at 64 drones x 4096 envs.

  scan:  microseconds per rvo3d_safety_scan (BatchedDroneEnv.safety, all four outputs) on the state some auto-resetting
         steps left, without buildings and with 50 buildings per env (per-env sets); device events around `--calls`
         back-to-back calls.
  eval:  ms per fused evaluation step (post_train, fused=True, the "mlp" policy kernel) with safety=False and with
         safety=True, timed as tools/bench_eval.py times it (the env's step is wrapped to start and stop the clock).

The set-ups alternate in one process, `--rounds` times, so the run-to-run spread shows next to the differences.  One
JSON line per run, then a summary line.  The safety=False loop is tools/bench_eval.py's `fused:mlp` variant: to compare
it with another commit, alternate `tools/bench_eval.py --only fused:mlp --rounds 1` between the two checkouts."""
import argparse, json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd"))
from rvo3d_amd import BatchedDroneEnv, synthetic_actions, synthetic_world
from rvo3d_amd.policy import mlp_ac, post_train

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--drones", type=int, default=64)
ap.add_argument("--buildings", type=int, default=50)
ap.add_argument("--calls", type=int, default=200, help="timed scans per run")
ap.add_argument("--steps", type=int, default=200, help="timed evaluation steps per run")
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--poll-every", type=int, default=8)
ap.add_argument("--only", default=None, choices=("scan", "eval"))
args = ap.parse_args()
E, N = args.envs, args.drones
MAP = (50, 50, 10)
worlds = {"nb0": synthetic_world(E, N, MAP), f"nb{args.buildings}": synthetic_world(E, N, MAP, nb=args.buildings,
                                                                                  per_env_buildings=True)}


def scan_us(world):
    env = BatchedDroneEnv(world)
    for t in range(20):   # spread the drones: the state of a rollout, not the reset state
        env.step(torch.from_numpy(synthetic_actions(E, N, t)).cuda(), autoreset=True)
    for _ in range(args.warmup):
        env.safety(0.5)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.calls):
        env.safety(0.5)
    t1.record()
    torch.cuda.synchronize()
    near = int(env.safety(0.5)[3].sum().item())
    env.close()
    return t0.elapsed_time(t1) / args.calls * 1e3, near


class _Stop(Exception):
    pass


def eval_ms(safety):
    env = BatchedDroneEnv(worlds["nb0"])
    torch.manual_seed(0)
    ac = mlp_ac(env.W).cuda()
    pt = post_train(env, num_episodes=E * (args.warmup + args.steps + 8), max_ep_len=150, acceler_vel=1.0, inf_print=False,
                    std_factor=0.5, fused=True, policy_kernel="mlp", poll_every=args.poll_every, safety=safety)
    plain_step, n, t = env.step, [0], [0.0, 0.0]

    def step(action, autoreset=False):
        if n[0] in (args.warmup, args.warmup + args.steps):
            torch.cuda.synchronize()
            t[n[0] > args.warmup] = time.perf_counter()
            if n[0] > args.warmup:
                raise _Stop
        n[0] += 1
        return plain_step(action, autoreset)

    env.step = step
    try:
        pt.policy_test(policy=ac)
        raise RuntimeError("the evaluation ended before the timed steps did")
    except _Stop:
        pass
    env.close()
    return (t[1] - t[0]) / args.steps * 1e3


out = {"envs": E, "drones": N, "scan_us": {k: [] for k in worlds}, "eval_ms": {"safety_off": [], "safety_on": []}}
for r in range(args.rounds):
    if args.only in (None, "scan"):
        for k, w in worlds.items():
            us, near = scan_us(w)
            out["scan_us"][k].append(round(us, 2))
            print(json.dumps({"scan": k, "round": r, "us_per_scan": round(us, 2), "near_pairs": near}), flush=True)
    if args.only in (None, "eval"):
        for k, s in (("safety_off", False), ("safety_on", True)):
            out["eval_ms"][k].append(round(eval_ms(s), 4))
            print(json.dumps({"eval": k, "round": r, "ms_per_eval_step": out["eval_ms"][k][-1]}), flush=True)
print(json.dumps(out))
