"""Secondary measurement: ms per EVALUATION step (rvo3d_amd.policy.post_train.policy_test) at 64 drones x 4096 envs with
the MLP(256, 256) actor-critic, for the unfused loop (module policy) and the fused loop with the module policy, the
"mlp" kernel and the "mlp_x3" kernel.  The variants alternate in one process, `--rounds` times, so the run-to-run spread
shows next to the differences; a run warms up, then times `--steps` steps between two synchronisations.  The loop has no
step limit of its own: the env's step is wrapped to stop it.  One JSON line per run, then a summary line.

Per-kernel times and launches per step of one variant:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_eval.py --only fused:mlp --rounds 1
(a run of its own: the trace slows the host side down)."""
import argparse, json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd"))
from rvo3d_amd import BatchedDroneEnv, synthetic_world
from rvo3d_amd.policy import mlp_ac, post_train

VARIANTS = ("unfused:module", "fused:module", "fused:mlp", "fused:mlp_x3")
ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--drones", type=int, default=64)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--poll-every", type=int, default=8)
ap.add_argument("--only", default=None, help="one of " + ", ".join(VARIANTS))
args = ap.parse_args()
E, N = args.envs, args.drones
world = synthetic_world(E, N, (50, 50, 10))


class _Stop(Exception):
    pass


def run(variant):
    loop, kernel = variant.split(":")
    env = BatchedDroneEnv(world)
    torch.manual_seed(0)
    ac = mlp_ac(env.W).cuda()
    # a quota no env can fill in the timed steps (an episode takes a step at least): the loop runs until the wrapped
    # step stops it.  (With this untrained policy some env ends an episode in nearly every step.)
    pt = post_train(env, num_episodes=E * (args.warmup + args.steps + 8), max_ep_len=150, acceler_vel=1.0, inf_print=False, std_factor=0.5,
                    fused=loop == "fused", policy_kernel=None if kernel == "module" else kernel,
                    poll_every=args.poll_every)
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


variants = (args.only,) if args.only else VARIANTS
if any(v not in VARIANTS for v in variants):
    raise SystemExit("--only must be one of " + ", ".join(VARIANTS))
ms = {v: [] for v in variants}
for r in range(args.rounds):
    for v in variants:
        ms[v].append(run(v))
        print(json.dumps({"variant": v, "round": r, "envs": E, "drones": N, "steps": args.steps,
                          "ms_per_eval_step": round(ms[v][-1], 4)}), flush=True)
print(json.dumps({"envs": E, "drones": N, "steps": args.steps, "poll_every": args.poll_every,
                  "ms_per_eval_step": {v: [round(x, 4) for x in xs] for v, xs in ms.items()}}))
