#!/usr/bin/env python3
"""usage: tools/policy_mlp_x3_check.py [--rows 262144] [--width 102] [--iters 50]
Config 3's policy step three ways, in one process, on the same rows (env-shaped: 12 state floats, 9 per kept VO row,
zeros behind; 10 % of the rows carry VO rows; the env's counts passed where the kernel takes them) and the same
default-initialised MLP(256, 256): the bf16 kernel (rvo3d_policy_mlp_sample), the split-bf16 kernel
(rvo3d_policy_mlp_x3_sample) and the float32 "heads" path (float32 GEMMs up to the last hidden layers +
rvo3d_policy_sample, as multi_ppo runs it with amp=False).  Prints one JSON line per path: error of mu (before the
tanh; heads path: after it, against tanh of the float64 forward) and v against a float64 forward, and us per call
(HIP events, mean over --iters calls after warm-up).  Not part of the product path."""
import argparse, ctypes as C, json, os, sys
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd"), os.path.join(ROOT, "tests")]
from rvo3d_amd import _lib
from rvo3d_amd.policy import mlp_ac
from test_policy_x3_host import config3_like_obs, forward64

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=64 * 4096)
ap.add_argument("--width", type=int, default=102)
ap.add_argument("--iters", type=int, default=50)
args = ap.parse_args()
W, B, dev = args.width, args.rows, "cuda"
L = _lib.lib()
torch.manual_seed(0)
ac = mlp_ac(W).to(dev)
x, cnt = config3_like_obs(B, W, seed=1)
x, cnt = x.to(dev), cnt.to(dev)
with torch.no_grad():
    z64, v64 = forward64(ac.pi_net[:-1], x), forward64(ac.v_net, x).squeeze(-1)
out = [torch.zeros(s, device=dev) for s in ((B, 3), (B,), (B,), (B, 3), (B, 3))]
p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.iters


def kernel(precision):
    mb = ac.mlp_blob(precision)
    f = L.rvo3d_policy_mlp_sample if precision == "bf16" else L.rvo3d_policy_mlp_x3_sample

    def call(tanh=1, dbg=False):
        _lib.check(f(p(mb["blob"]), W, p(x), x.stride(0), B, p(cnt), 12, 9, tanh, p(ac.log_std), 1.0, 7, 0,
                     p(out[0]), p(out[1]), p(out[2]), p(out[3]) if dbg else None, None, st()), precision)
    us = timed(call)
    call(tanh=0, dbg=True)
    torch.cuda.synchronize()
    return us, out[3].double(), out[2].double(), "pre-tanh"


def heads():
    plan = ac.fused_plan(torch.float32)
    cache = {}

    def call(dbg=False):
        xc = ac.prepare_input(x, cnt, plan, cache)
        with torch.no_grad():
            hp, hv = ac.hidden_pair(xc, plan)
        hd = _lib.PolicyHeads(hp.data_ptr(), hv.data_ptr(), hp.stride(0), hv.stride(0), _lib.RVO3D_F32, plan["hidden"],
                              1 if plan["tanh"] else 0, 0, plan["w_pi"].data_ptr(), plan["b_pi"].data_ptr(),
                              plan["w_v"].data_ptr(), plan["b_v"].data_ptr(), ac.log_std.data_ptr())
        _lib.check(L.rvo3d_policy_sample(C.byref(hd), B, 1.0, 7, 0, p(out[0]), p(out[1]), p(out[2]),
                                         p(out[3]) if dbg else None, None, st()), "heads")
    us = timed(call)
    call(dbg=True)
    torch.cuda.synchronize()
    return us, out[3].double(), out[2].double(), "after tanh"


with torch.no_grad():
    z64 = forward64(ac.pi_net, x)            # pre-tanh
res = {}
for name, fn in (("bf16", lambda: kernel("bf16")), ("x3", lambda: kernel("x3")), ("fp32_heads", heads)):
    us, mu, v, kind = fn()
    ref = z64 if kind == "pre-tanh" else torch.tanh(z64)
    d_mu, d_v = (mu - ref).abs(), (v - v64).abs()
    res[name] = us
    print(json.dumps({"path": name, "rows": B, "width": W, "us_per_call": round(us, 1), "mu": kind,
                      "mu_err_max": float(d_mu.max()), "mu_err_mean": float(d_mu.mean()),
                      "v_err_max": float(d_v.max()), "v_err_rel_max": float((d_v / v64.abs().clamp(min=1)).max()),
                      "vo_share": float((cnt > 0).float().mean())}), flush=True)
print(json.dumps({"x3_over_bf16": res["x3"] / res["bf16"], "x3_over_fp32_heads": res["x3"] / res["fp32_heads"]}))
