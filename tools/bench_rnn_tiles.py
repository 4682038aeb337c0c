"""The biGRU actor-critic's policy step in a world with velocity obstacles (the classical swap scene,
rvo3d_amd.worlds.crossing_world): E envs x N drones fly at their desired velocity (env.des_vel()) towards the antipodal
destination for --warm steps; along the way the tool records the fraction of observation rows with VO rows and the
histogram of vo_count.  On --snapshots observation sets of the timed window it then times, with HIP events:
  tiles  - rvo3d_policy_rnn_tiles on the rows that have VO rows (the list rvo3d_reader_zero_features builds);
  rows   - rvo3d_policy_rows on the same list (one workgroup per row and network);
  heads  - the library-GEMM "heads" path on every row (rnn_ac.prepare_input + hidden_pair + rvo3d_policy_sample);
and a full rollout step (multi_ppo.collect, amp) in modes "rnn_tiles" and "heads" from the warmed state.
--fp32: the float32 rollout instead - rvo3d_policy_rnn_tiles_x3 next to the bf16 kernel on the same lists (and the two
collapsed zero-VO layers), then a rollout step of multi_ppo(amp=False, fused_rnn_fp32=True), "rnn_tiles_x3", and of the
amp=False path it replaces, "heads", in the same run; on the crossing world and on synthetic_world(envs, drones,
(50, 50, 10)), the benchmark's sparse world.
One JSON line per measurement (--out appends them to a file as well).  Not the bench.py headline."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd"))
from rvo3d_amd import BatchedDroneEnv, _lib, crossing_world, synthetic_world  # noqa: E402
from rvo3d_amd.policy import multi_ppo, rnn_ac  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--drones", type=int, default=64)
ap.add_argument("--map", type=float, nargs=3, default=(30.0, 30.0, 10.0))
ap.add_argument("--radius", type=float, default=None, help="ring radius (default 0.4 min(L, W))")
ap.add_argument("--alt-spread", type=float, default=1.0)
ap.add_argument("--warm", type=int, default=20, help="des_vel steps before the timed window")
ap.add_argument("--snapshots", type=int, default=4, help="observation sets of the timed window (one per step)")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rollout-steps", type=int, default=8)
ap.add_argument("--hidden", type=int, default=256)
ap.add_argument("--skip-rows", action="store_true", help="leave out rvo3d_policy_rows (slow at high density)")
ap.add_argument("--fp32", action="store_true", help="the float32-class kernels and rollout modes, on both worlds")
ap.add_argument("--out", default=None)
args = ap.parse_args()
E, N = args.envs, args.drones
dev = torch.device("cuda")
L = _lib.lib()


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def p(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, before=None, reps=args.reps):
    """median / min milliseconds of fn() over reps, HIP events around fn alone (before() runs outside them)."""
    ts = []
    for _ in range(reps + 1):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts = ts[1:]
    return float(np.median(ts)), float(np.min(ts))


class Space:
    shape = (3,)


def measure(world, world_name, map_size):
    env = BatchedDroneEnv(world)
    env.reset(); env.observe()
    W, nm = env.W, env.nm
    dens = []
    for t in range(args.warm):
        env.step(env.des_vel(), autoreset=True)
        dens.append(float((env.vo_count > 0).float().mean()))
    snaps = []
    for t in range(args.snapshots):
        env.step(env.des_vel(), autoreset=True)
        snaps.append((env.obs.reshape(E * N, W).clone(), env.vo_count.reshape(E * N).clone()))
    state = env.state_dict()
    win = [float((c > 0).float().mean()) for _, c in snaps]
    hist = np.bincount(torch.cat([c for _, c in snaps]).cpu().numpy(), minlength=nm + 1).tolist()
    emit(dict(what="density", world=world_name, envs=E, drones=N, map=list(map_size), radius=args.radius, alt_spread=args.alt_spread,
              warm=args.warm, frac_vo_rows_warm=[round(x, 4) for x in dens], frac_vo_rows_window=[round(x, 4) for x in win],
              vo_count_hist_window=hist))


    torch.manual_seed(0)
    ac = rnn_ac(None, Space(), 12, 9, args.hidden, (256, 256), (256, 256), torch.nn.ReLU, torch.nn.Tanh, torch.nn.Identity,
                use_gpu=False, rnn_mode="biGRU").cuda()
    zp, tb = ac.zero_vo_plan(), ac.rnn_tiles_blob()
    zp3, tb3 = (ac.zero_vo_plan("x3"), ac.rnn_tiles_blob("x3")) if args.fp32 else (None, None)
    B = E * N
    f0 = torch.empty((B, zp["width"]), device=dev)
    lst = torch.zeros(B, dtype=torch.int32, device=dev)
    ctr = torch.zeros(2, dtype=torch.int32, device=dev)
    work = torch.zeros(int(L.rvo3d_policy_rnn_tiles_work_bytes(B, nm)) // 4, dtype=torch.int32, device=dev)
    act = torch.empty((B, 3), device=dev); logp = torch.empty(B, device=dev); val = torch.empty(B, device=dev)
    log_std = ac.log_std.detach()
    net = zp["rows_net"]; net.slots = nm
    plan = ac.fused_plan(torch.bfloat16)
    cache = {}

    # issued MFMA work of the tiles kernel for a count histogram (v_mfma_f32_32x32x16_bf16 = 32768 flop)
    H, ND = args.hidden, 2
    HT, KH = H // 32, H // 16


    def tiles_mfma(hist_one):
        n = 0
        for c, k in enumerate(hist_one):
            if c == 0 or k == 0:
                continue
            tiles = (k + 31) // 32
            gru = ND * (3 * HT * 3 + (c - 1) * 3 * HT * KH * 3)
            heads = 2 * (8 * (KH + 1) + 8 * 16 + 16)
            n += tiles * (gru + heads)
        return n


    for si, (x, cnt) in enumerate(snaps):
        def build_list():
            _lib.check(L.rvo3d_reader_zero_features(p(x), W, B, zp["state_dim"], zp["feat_dim"], p(zp["ln_w"]), p(zp["ln_b"]),
                                                    zp["sum_h0"], zp["sumsq_h0"], zp["eps"], p(f0), f0.stride(0), p(cnt),
                                                    p(lst), p(ctr), stream()), "rvo3d_reader_zero_features")

        def tiles():
            _lib.check(L.rvo3d_policy_rnn_tiles(p(tb["blob"]), tb["blob_bytes"], tb["hidden"], 9, 12, 1, p(x), W, p(cnt), p(lst),
                                                p(ctr), C.c_void_p(ctr.data_ptr() + 4), p(work), B, nm, 1, p(log_std), 1.0, 7,
                                                si, p(act), p(logp), p(val), None, stream()), "rvo3d_policy_rnn_tiles")

        def tiles_x3():
            _lib.check(L.rvo3d_policy_rnn_tiles_x3(p(tb3["blob"]), tb3["blob_bytes"], tb3["hidden"], 9, 12, 1, p(x), W, p(cnt),
                                                   p(lst), p(ctr), C.c_void_p(ctr.data_ptr() + 4), p(work), B, nm, 1,
                                                   p(log_std), 1.0, 7, si, p(act), p(logp), p(val), None, stream()),
                       "rvo3d_policy_rnn_tiles_x3")

        def zero_part_x3():
            build_list()
            _lib.check(L.rvo3d_policy_mlp_x3_sample(p(zp3["blob"]), zp3["width"], p(f0), f0.stride(0), B, None, 0, 0, 1,
                                                    p(log_std), 1.0, 7, si, p(act), p(logp), p(val), None, None, stream()),
                       "rvo3d_policy_mlp_x3_sample")

        def rows():
            _lib.check(L.rvo3d_policy_rows(C.byref(net), p(x), W, p(cnt), p(lst), p(ctr), C.c_void_p(ctr.data_ptr() + 4), 1,
                                           p(log_std), 1.0, 7, si, p(act), p(logp), p(val), stream()), "rvo3d_policy_rows")

        def zero_part():
            build_list()
            _lib.check(L.rvo3d_policy_mlp_sample(p(zp["blob"]), zp["width"], p(f0), f0.stride(0), B, None, 0, 0, 1, p(log_std),
                                                 1.0, 7, si, p(act), p(logp), p(val), None, None, stream()),
                       "rvo3d_policy_mlp_sample")

        def heads():
            with torch.no_grad():
                xc = ac.prepare_input(x, cnt, plan, cache)
                hp, hv = ac.hidden_pair(xc, plan)
            hd = _lib.PolicyHeads(hp.data_ptr(), hv.data_ptr(), hp.stride(0), hv.stride(0), _lib.RVO3D_BF16, plan["hidden"], 1,
                                  0, plan["w_pi"].data_ptr(), plan["b_pi"].data_ptr(), plan["w_v"].data_ptr(),
                                  plan["b_v"].data_ptr(), log_std.data_ptr())
            _lib.check(L.rvo3d_policy_sample(C.byref(hd), B, 1.0, 7, si, p(act), p(logp), p(val), None, None, stream()),
                       "rvo3d_policy_sample")

        h1 = np.bincount(cnt.cpu().numpy(), minlength=nm + 1)
        n_list = int((cnt > 0).sum())
        t_tiles = timed(tiles, build_list)
        flop = tiles_mfma(h1) * 32768
        rec = dict(what="policy_kernels", world=world_name, snapshot=si, rows=B, listed=n_list, frac_vo_rows=round(n_list / B, 4),
                   vo_count_hist=h1.tolist(), tiles_us=round(t_tiles[0] * 1e3, 1), tiles_min_us=round(t_tiles[1] * 1e3, 1),
                   tiles_mfma_tflops=round(flop / (t_tiles[0] * 1e-3) / 1e12, 1),
                   tiles_mfma_frac_of_peak=round(flop / (t_tiles[0] * 1e-3) / 2.5e15, 4),
                   zero_vo_part_us=round(timed(zero_part)[0] * 1e3, 1))
        if args.fp32:   # (the issued MFMA work of the x3 stacks is three times the bf16 stacks'; the GRU's is the same)
            t_x3 = timed(tiles_x3, build_list)
            rec.update(tiles_x3_us=round(t_x3[0] * 1e3, 1), tiles_x3_min_us=round(t_x3[1] * 1e3, 1),
                       zero_vo_part_x3_us=round(timed(zero_part_x3)[0] * 1e3, 1))
        else:
            if not args.skip_rows:
                rec["rows_us"] = round(timed(rows, build_list, reps=3)[0] * 1e3, 1)
            rec["heads_us"] = round(timed(heads)[0] * 1e3, 1)
        emit(rec)

    # full rollout steps from the warmed state
    modes = ((dict(fused_rnn_fp32=True), "rnn_tiles_x3"), (dict(), "heads")) if args.fp32 else \
        ((dict(fused_rnn_tiles=True), "rnn_tiles"), (dict(fused_mlp=False), "heads"))
    for mode_kw, name in modes:
        T = args.rollout_steps
        tr = multi_ppo(env, ac, train_epoch=0, steps_per_epoch=T, max_ep_len=500, save_freq=10**9, amp=not args.fp32,
                       **mode_kw)
        assert tr._fused_mode() == name, tr._fused_mode()
        ts, fr = [], []
        for rep in range(3):
            env.load_state_dict(state); env.observe()
            tr._cur = (env.obs, env.vo_count)   # (start every rollout from the warmed state)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            tr.collect()
            torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) / T * 1e3)
            fr.append(float((tr.buf.cnt[:T] > 0).float().mean()))
        emit(dict(what="rollout_step", world=world_name, mode=name, amp=not args.fp32, envs=E, drones=N, steps=T, ms_per_step=[round(v, 3) for v in ts],
                  frac_vo_rows=[round(v, 4) for v in fr]))
    del tr
    env.close()


measure(crossing_world(E, N, tuple(args.map), radius=args.radius, alt_spread=args.alt_spread, seed=1), "crossing", args.map)
if args.fp32:
    measure(synthetic_world(E, N, (50.0, 50.0, 10.0)), "synthetic_50x50x10", (50.0, 50.0, 10.0))
