#!/usr/bin/env python3
"""usage: tools/ab_rollout_precision.py [--epochs 20] [--envs 32] [--drones 16] [--steps 64]
The same PPO run (same seed, same small world, same initial weights) three ways: bf16 rollouts (amp=True, the bf16
policy kernel), float32 rollouts through the split-bf16 kernel (fused_mlp_fp32=True, mode mlp_x3) and float32
rollouts through float32 GEMMs + the heads kernel (mode heads).  One JSON line per epoch and mode: mean return of the
episodes that ended, approx-KL of the first and the last policy iteration of the update (the first one measures how
far the rollout's stored log-probabilities sit from the module's own).  Not part of the product path."""
import argparse, json, os, sys
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3drvo-marl-collisionavoidance_amd"))
from rvo3d_amd import BatchedDroneEnv, synthetic_world
from rvo3d_amd.policy import mlp_ac, multi_ppo

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=20)
ap.add_argument("--envs", type=int, default=32)
ap.add_argument("--drones", type=int, default=16)
ap.add_argument("--steps", type=int, default=64)
args = ap.parse_args()
world = synthetic_world(args.envs, args.drones, (12, 12, 6), n_points=3, seed=5)
for name, kw in (("bf16", dict(amp=True)), ("x3", dict(amp=False, fused_mlp_fp32=True)), ("fp32_heads", dict(amp=False))):
    env = BatchedDroneEnv(world)
    torch.manual_seed(0)
    ac = mlp_ac(env.W).cuda()
    tr = multi_ppo(env, ac, steps_per_epoch=args.steps, max_ep_len=100, train_pi_iters=10, train_v_iters=10,
                   target_kl=1e9, seed=3, tune_gemms=False, **kw)
    env.reset(); env.observe()
    for ep in range(args.epochs):
        tr.buf.ptr = 0
        ret = tr.collect()
        data = tr.buf.get()
        kl = []
        orig = tr.compute_loss_pi

        def rec(d, _orig=orig):
            out = _orig(d)
            kl.append(float(out[1]["kl"]))
            return out
        tr.compute_loss_pi = rec
        tr.update(data)
        tr.compute_loss_pi = orig
        print(json.dumps({"mode": name, "fused_mode": tr._fused_mode(), "epoch": ep, "mean_return": ret,
                          "approx_kl_first_iter": kl[0] if kl else None, "approx_kl_last_iter": kl[-1] if kl else None}),
              flush=True)
    env.close()
