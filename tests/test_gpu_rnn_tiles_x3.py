"""The float32-class policy step of the biGRU actor-critic: rvo3d_policy_rnn_tiles_x3 (the rows WITH velocity-obstacle
rows; csrc/rvo3d_policy_rnn_tiles.hpp, X3 = true), zero_vo_plan("x3") on rvo3d_policy_mlp_x3_sample (the rows without),
the trainer mode built on them (multi_ppo(amp=False, fused_rnn_fp32=True), "rnn_tiles_x3") and the evaluator's
policy_kernel "rnn_tiles" / "rnn_tiles_x3".  Accuracy is measured against a float64 forward of the modules within the
bounds of tests/test_policy_x3_host.py (the bf16 kernels on the same rows fall outside them: tests/test_rnn_x3_host.py
has the error model); isolation, list protocol and sampling as tests/test_gpu_rnn_tiles.py checks them for bf16."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from golden_util import load
from rvo3d_amd import BatchedDroneEnv, _lib, crossing_world, synthetic_world
from rvo3d_amd.policy import mlp_ac, multi_ppo, post_train
from test_gpu_parity import world_of
from test_gpu_policy_x3 import _account_replay
from test_gpu_rnn_tiles import _ac, _p, _rows, _stream
from test_policy_x3_host import MU_MAX, MU_MEAN, V_REL, config3_like_obs

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _names(precision):
    return ("rvo3d_policy_mlp_x3_sample", "rvo3d_policy_rnn_tiles_x3") if precision == "x3" else \
        ("rvo3d_policy_mlp_sample", "rvo3d_policy_rnn_tiles")


class Tiles:
    """One set of buffers for rvo3d_policy_rnn_tiles / _x3 over `rows` observation rows."""

    def __init__(self, ac, rows, nm, precision="x3"):
        self.tb = ac.rnn_tiles_blob(precision)
        assert self.tb is not None
        self.rows, self.nm, self.fn = rows, nm, getattr(_lib.lib(), _names(precision)[1])
        self.work = torch.zeros(int(_lib.lib().rvo3d_policy_rnn_tiles_work_bytes(rows, nm)) // 4, dtype=torch.int32,
                                device=DEV)
        self.lst = torch.zeros(rows, dtype=torch.int32, device=DEV)
        self.ctr = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.log_std = ac.log_std.detach()

    def __call__(self, obs, cnt, listed, seed=7, step=3):
        tb, rows = self.tb, self.rows
        n = int(listed.numel())
        self.lst[:n] = listed.to(torch.int32)
        self.ctr[0] = n
        act = torch.full((rows, 3), 9.0, device=DEV)
        logp = torch.full((rows,), 9.0, device=DEV)
        val = torch.full((rows,), 9.0, device=DEV)
        mu = torch.full((rows, 3), 9.0, device=DEV)
        _lib.check(self.fn(
            _p(tb["blob"]), tb["blob_bytes"], tb["hidden"], tb["in_dim"], tb["state_dim"], tb["bidir"], _p(obs),
            obs.stride(0), _p(cnt), _p(self.lst), _p(self.ctr), C.c_void_p(self.ctr.data_ptr() + 4), _p(self.work),
            rows, self.nm, 1 if tb["tanh"] else 0, _p(self.log_std), 1.0, seed, step, _p(act), _p(logp), _p(val), _p(mu),
            _stream()), "rvo3d_policy_rnn_tiles")
        torch.cuda.synchronize()
        return act, logp, val, mu

    def clean(self):
        return self.ctr.tolist() == [0, 0] and int(self.work[:32].abs().sum()) == 0


def _forward64(ac, obs, cnt):
    """(mu through the actor's own output activation, v) of the modules in float64."""
    a64 = copy.deepcopy(ac).double()
    with torch.no_grad():
        f = a64.pi.rnn_reader.forward_batch(obs.double(), torch.clamp(cnt.long(), min=1))
        return a64.pi.net_out(f), a64.v.v_net(f).squeeze(-1)


def _figures(mu, val, mu64, v64):
    d_mu, d_v = (mu.double() - mu64).abs(), (val.double() - v64).abs()
    ok = (float(d_mu.max()) <= MU_MAX and float(d_mu.mean()) <= MU_MEAN
          and bool((d_v <= V_REL * v64.abs().clamp(min=1.0)).all()))
    return ok, (float(d_mu.max()), float(d_mu.mean()), float(d_v.max()))


# ---- 1. accuracy, rows with VO rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,bi", [(256, True), (256, False), (64, True), (64, False)])
def test_x3_tiles_accuracy_against_float64(hidden, bi):
    nm, rows, n_list = 12, 1001, 401   # (401 listed rows: 34 of counts 1..5, 33 of 6..12 - every last tile is ragged)
    ac = _ac(hidden, bi, 5 + hidden + bi)
    obs, cnt, pick = _rows(rows, nm, n_list, 11)
    per_count = torch.bincount(cnt[pick].long(), minlength=nm + 1)[1:]
    assert bool((per_count > 0).all()) and bool((per_count % 32 != 0).all())
    mu64, v64 = _forward64(ac, obs[pick], cnt[pick])
    untouched = torch.ones(rows, dtype=torch.bool, device=DEV)
    untouched[pick] = False
    for precision in ("x3", "bf16"):
        out = Tiles(ac, rows, nm, precision)(obs, cnt, pick)
        act, logp, val, mu = out
        ok, fig = _figures(mu[pick], val[pick], mu64, v64)
        print(f"hidden {hidden} bi {bi} {precision}: mu max {fig[0]:.2e} mean {fig[1]:.2e}, v max {fig[2]:.2e}")
        for t in out:   # the unlisted rows keep their sentinels
            assert bool((t[untouched] == 9.0).all()) and bool(torch.isfinite(t[pick]).all())
        if precision == "x3":
            assert ok, fig
        else:           # the bf16 stacks on the same rows: outside
            assert not ok, fig


# ---- 2. accuracy, zero-VO rows ----------------------------------------------------------------------------------------
def _zero_vo(ac, precision, x, std_factor=1.0, seed=7, step=3):
    """rvo3d_reader_zero_features + the MLP kernel on zero_vo_plan(precision): act, logp, val, mu."""
    L, zp, rows = _lib.lib(), ac.zero_vo_plan(precision), x.shape[0]
    assert zp is not None and (zp["rows_net"] is None or precision == "bf16")
    feat = torch.empty((rows, zp["width"]), device=DEV)
    _lib.check(L.rvo3d_reader_zero_features(_p(x), x.stride(0), rows, zp["state_dim"], zp["feat_dim"], _p(zp["ln_w"]),
                                            _p(zp["ln_b"]), zp["sum_h0"], zp["sumsq_h0"], zp["eps"], _p(feat),
                                            feat.stride(0), None, None, None, _stream()), "rvo3d_reader_zero_features")
    out = [torch.empty(s, device=DEV) for s in ((rows, 3), (rows,), (rows,), (rows, 3))]
    name = _names(precision)[0]
    _lib.check(getattr(L, name)(_p(zp["blob"]), zp["width"], _p(feat), feat.stride(0), rows, None, 0, 0,
                                1 if zp["tanh"] else 0, _p(ac.log_std), std_factor, seed, step, *[_p(t) for t in out],
                                None, _stream()), name)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("hidden,bi", [(256, True), (64, False)])
def test_x3_zero_vo_plan_accuracy_against_float64(hidden, bi):
    ac = _ac(hidden, bi, 50 + hidden)
    x, cnt = config3_like_obs(4001, 102, vo_share=0.0, seed=hidden)
    x, cnt = x.to(DEV), cnt.to(DEV)
    mu64, v64 = _forward64(ac, x, cnt)
    for precision in ("x3", "bf16"):
        _, _, val, mu = _zero_vo(ac, precision, x)
        ok, fig = _figures(mu, val, mu64, v64)
        print(f"zero-VO hidden {hidden} {precision}: mu max {fig[0]:.2e} mean {fig[1]:.2e}, v max {fig[2]:.2e}")
        if precision == "x3":
            assert ok, fig
        else:
            assert not ok, fig
    # one cache entry per precision, repacked in place when a parameter changed
    z3 = ac.zero_vo_plan("x3")
    assert ac.zero_vo_plan("x3") is z3 and ac.zero_vo_plan() is not z3
    assert z3["blob"].numel() == _lib.lib().rvo3d_policy_mlp_x3_blob_bytes(z3["width"])
    with torch.no_grad():
        ac.pi.net_out[0].bias.add_(1.0)
    assert ac.zero_vo_plan("x3") is not z3 and ac.zero_vo_plan("x3")["blob"].data_ptr() == z3["blob"].data_ptr()


# ---- 3. isolation and protocol ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [256, 64])
def test_x3_tiles_isolation_and_list_protocol(hidden):
    nm, rows = 10, 1200
    ac = _ac(hidden, True, 21)
    obs, cnt, pick = _rows(rows, nm, 413, 12)
    run = Tiles(ac, rows, nm)
    ref = run(obs, cnt, pick)
    assert run.clean()
    got = run(obs, cnt, pick[torch.randperm(pick.numel(), device=DEV)])
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    assert run.clean()
    for k in (1, 2, nm):   # one count alone against the same rows mixed with every other count
        sub = pick[cnt[pick] == k]
        alone = run(obs, cnt, sub)
        others = torch.ones(rows, dtype=torch.bool, device=DEV)
        others[sub] = False
        for a, b in zip(ref, alone):
            assert torch.equal(a[sub], b[sub]) and bool((b[others] == 9.0).all())
        assert run.clean()
    out = run(obs, cnt, pick[:0])   # an empty list
    assert all(bool((t == 9.0).all()) for t in out) and run.clean()


# ---- 4. sampling ------------------------------------------------------------------------------------------------------
def test_x3_tiles_sampling_is_rvo3d_policy_sample():
    nm, rows = 10, 900
    ac = _ac(256, True, 31)
    obs, cnt, pick = _rows(rows, nm, 301, 13)
    run = Tiles(ac, rows, nm)
    for seed, step in ((7, 3), (12345, 1 << 33)):
        act, logp, val, mu = run(obs, cnt, pick, seed=seed, step=step)
        a2 = torch.empty((rows, 3), device=DEV); l2 = torch.empty(rows, device=DEV); v2 = torch.empty(rows, device=DEV)
        hd = _lib.PolicyHeads(mu.data_ptr(), val.data_ptr(), 3, 1, _lib.RVO3D_F32, 0, 0, 0, None, None, None, None,
                              ac.log_std.data_ptr())
        _lib.check(_lib.lib().rvo3d_policy_sample(C.byref(hd), rows, 1.0, seed, step, _p(a2), _p(l2), _p(v2), None, None,
                                                  _stream()), "rvo3d_policy_sample")
        torch.cuda.synchronize()
        assert torch.equal(act[pick], a2[pick]) and torch.equal(logp[pick], l2[pick]) and torch.equal(val[pick], v2[pick])


# ---- 5. cross-precision blobs -----------------------------------------------------------------------------------------
def test_blobs_of_the_other_precision_are_refused_without_a_launch():
    ac = _ac(64, True, 41)
    t3, tb = ac.rnn_tiles_blob("x3"), ac.rnn_tiles_blob()
    assert ac.rnn_tiles_blob("x3") is t3 and t3 is not tb and t3["blob_bytes"] > tb["blob_bytes"]
    assert t3["blob"].data_ptr() != tb["blob"].data_ptr()
    with torch.no_grad():
        ac.pi.net_out[0].bias.add_(1.0)
    t3b = ac.rnn_tiles_blob("x3")
    assert t3b is not t3 and t3b["blob"].data_ptr() == t3["blob"].data_ptr()
    L = _lib.lib()
    rows, nm = 64, 4
    obs, cnt, pick = _rows(rows, nm, 10, 1)
    run = Tiles(ac, rows, nm)
    run.lst[:10] = pick.to(torch.int32)
    run.ctr[0] = 10
    o = torch.full((rows * 5,), 9.0, device=DEV)
    args = lambda b: (_p(b["blob"]), b["blob_bytes"], 64, 9, 12, 1, _p(obs), obs.stride(0), _p(cnt), _p(run.lst),
                      _p(run.ctr), C.c_void_p(run.ctr.data_ptr() + 4), _p(run.work), rows, nm, 1, _p(run.log_std), 1.0,
                      7, 0, _p(o), _p(o), _p(o), None, None)
    assert L.rvo3d_policy_rnn_tiles_x3(*args(tb)) == -1 and b"another" in L.rvo3d_last_error()
    assert L.rvo3d_policy_rnn_tiles(*args(t3b)) == -1 and b"another" in L.rvo3d_last_error()
    torch.cuda.synchronize()
    # nothing was launched: the list is still there, nothing was written
    assert run.ctr.tolist() == [10, 0] and bool((o == 9.0).all())
    assert L.rvo3d_policy_rnn_tiles_x3(*args(t3b)) == 0
    torch.cuda.synchronize()
    assert run.clean() and not bool((o == 9.0).all())


# ---- 6. the trainer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world_kind", ["dense", "crossing"])
def test_trainer_rnn_tiles_x3_mode_is_a_faithful_float32_rollout(world_kind):
    E, N, T = 64, 16, 24
    world = synthetic_world(E, N, (9, 9, 5), n_points=3, seed=4) if world_kind == "dense" else \
        crossing_world(E, N, (12, 12, 6), radius=4.0, alt_spread=0.5, seed=4)
    ac = _ac(256, True, 0)
    env = BatchedDroneEnv(world)
    assert multi_ppo(env, ac, steps_per_epoch=T, amp=False)._fused_mode() == "heads"   # (the flag off: what it was)
    tr = multi_ppo(env, ac, steps_per_epoch=T, max_ep_len=9, train_pi_iters=2, train_v_iters=2, amp=False, seed=3,
                   fused_rnn_fp32=True)
    assert tr._fused_mode() == "rnn_tiles_x3"
    env.reset(); env.observe()
    mean_ret = tr.collect()
    buf = tr.buf
    assert buf.ptr == T and tr._fused_mode() == "rnn_tiles_x3"
    frac = float((buf.cnt[:T] > 0).float().mean())
    print(f"{world_kind}: {frac:.4f} of the rows have VO rows")
    assert frac > (1e-3 if world_kind == "dense" else 0.0), frac
    _account_replay(world, buf, T, 9, mean_ret)

    def values_and_noise():
        with torch.no_grad():
            arg = (tr.buf.obs[:T].reshape(-1, env.W), tr.buf.cnt[:T].reshape(-1))
            d, _ = ac.pi(arg)
            v = ac.v(arg)
        got = tr.buf.val[:T].reshape(-1)
        assert torch.allclose(got, v, atol=1e-4, rtol=1e-4), float((got - v).abs().max())
        return (tr.buf.act[:T].reshape(-1, 3) - d.mean) / d.stddev

    z = values_and_noise()
    assert abs(float(z.mean())) < 0.02 and abs(float(z.var()) - 1) < 0.05
    # an update changes the weights; the next rollout runs on the repacked blobs, still in this mode
    blobs0 = [ac.zero_vo_plan("x3")["blob"].clone(), ac.rnn_tiles_blob("x3")["blob"].clone()]
    st = tr.update(buf.get())
    assert np.isfinite(st["loss_v"])
    assert not torch.equal(blobs0[0], ac.zero_vo_plan("x3")["blob"])
    assert not torch.equal(blobs0[1], ac.rnn_tiles_blob("x3")["blob"])
    tr.collect()
    assert tr._fused_mode() == "rnn_tiles_x3"
    values_and_noise()
    env.close()


def test_rnn_tiles_x3_mode_refuses_what_it_cannot_run():
    env = BatchedDroneEnv(synthetic_world(4, 8, (9, 9, 5), n_points=3, seed=4))
    with pytest.raises(ValueError, match="fused_rnn_fp32"):
        multi_ppo(env, _ac(256, True, 0), steps_per_epoch=4, amp=True, fused_rnn_fp32=True)
    with pytest.raises(ValueError, match="fused_rnn_fp32"):
        multi_ppo(env, _ac(256, True, 0, mode="LSTM"), steps_per_epoch=4, amp=False, fused_rnn_fp32=True)
    with pytest.raises(ValueError):   # (as before)
        multi_ppo(env, _ac(256, True, 0), steps_per_epoch=4, amp=False, fused_rnn_tiles=True)
    env.close()


# ---- 7. the evaluator -------------------------------------------------------------------------------------------------
def _three_launches(ac, precision, env, obs, cnt, std_factor, seed, step):
    """The evaluator's policy step by hand: rvo3d_reader_zero_features, the collapsed layer, the tiles.  Returns
    ([act, logp, val], number of listed rows)."""
    L, rows = _lib.lib(), obs.shape[0]
    zp, tb = ac.zero_vo_plan(precision), ac.rnn_tiles_blob(precision)
    slots = (env.W - 12) // 9
    feat = torch.empty((rows, zp["width"]), device=DEV)
    lst = torch.zeros(rows, dtype=torch.int32, device=DEV)
    ctr = torch.zeros(2, dtype=torch.int32, device=DEV)
    work = torch.zeros(int(L.rvo3d_policy_rnn_tiles_work_bytes(rows, slots)) // 4, dtype=torch.int32, device=DEV)
    out = [torch.empty(s, device=DEV) for s in ((rows, 3), (rows,), (rows,))]
    o = [_p(t) for t in out]
    tanh = 1 if zp["tanh"] else 0
    _lib.check(L.rvo3d_reader_zero_features(_p(obs), obs.stride(0), rows, zp["state_dim"], zp["feat_dim"], _p(zp["ln_w"]),
                                            _p(zp["ln_b"]), zp["sum_h0"], zp["sumsq_h0"], zp["eps"], _p(feat),
                                            feat.stride(0), _p(cnt), _p(lst), _p(ctr), _stream()), "zero features")
    listed = int(ctr[0])
    zero_mlp, tiles = _names(precision)
    _lib.check(getattr(L, zero_mlp)(_p(zp["blob"]), zp["width"], _p(feat), feat.stride(0), rows, None, 0, 0, tanh,
                                    _p(ac.log_std), std_factor, seed, step, *o, None, None, _stream()), zero_mlp)
    _lib.check(getattr(L, tiles)(_p(tb["blob"]), tb["blob_bytes"], tb["hidden"], tb["in_dim"], tb["state_dim"], tb["bidir"],
                                 _p(obs), obs.stride(0), _p(cnt), _p(lst), _p(ctr), C.c_void_p(ctr.data_ptr() + 4),
                                 _p(work), rows, slots, tanh, _p(ac.log_std), std_factor, seed, step, *o, None, _stream()),
               tiles)
    torch.cuda.synchronize()
    return out, listed


@pytest.mark.parametrize("kernel", ["rnn_tiles_x3", "rnn_tiles"])
def test_rnn_kernel_policy_in_both_loops(kernel):
    fx = load(os.path.join(GOLDEN, "post_train_world_8_train.npz"))
    precision = "x3" if kernel == "rnn_tiles_x3" else "bf16"
    got = {}
    for fused in (False, True):
        env = BatchedDroneEnv(world_of(fx), neighbors_num=10, env_train=True)
        ac = _ac(256, True, 3)
        pt = post_train(env, num_episodes=3, max_ep_len=12, acceler_vel=1.0, inf_print=False, std_factor=0.5,
                        fused=fused, policy_kernel=kernel, seed=11)
        got[fused] = pt.policy_test(policy=ac)
        env.close()
    assert got[True]["episodes"] == got[False]["episodes"] == 3
    for k in ("ep_len", "ep_ret", "success_rate", "mean_len", "std_len", "average_speed", "std_speed"):
        assert got[True][k] == got[False][k], k
    np.testing.assert_allclose(got[True]["speed"], got[False]["speed"], rtol=1e-12)

    # the first two policy calls against the three launches made by hand, noise steps 0 and 1
    env = BatchedDroneEnv(world_of(fx), neighbors_num=10, env_train=True)
    ac = _ac(256, True, 3)
    pt = post_train(env, num_episodes=3, max_ep_len=12, inf_print=False, std_factor=0.5, policy_kernel=kernel, seed=11)
    act_fn = pt.load_policy(ac, pt.std_factor)
    env.reset()
    obs, cnt = env.observe()
    obs, cnt = obs.view(-1, env.W), cnt.view(-1)
    first = act_fn(obs, cnt).clone()
    second = act_fn(obs, cnt).clone()
    for step, want in ((0, first), (1, second)):
        (mine, _, _), listed = _three_launches(ac, precision, env, obs, cnt, 0.5, 11, step)
        assert listed == int((cnt > 0).sum())
        assert torch.equal(mine.view(torch.int32), want.view(torch.int32)), step
    assert not torch.equal(first, second)    # (the call number is the noise step)
    env.close()


def test_rnn_kernel_policy_needs_the_rnn_actor_critic():
    fx = load(os.path.join(GOLDEN, "post_train_world_8_train.npz"))
    env = BatchedDroneEnv(world_of(fx), neighbors_num=10)
    mlp = mlp_ac(env.W).cuda()
    for kernel in ("rnn_tiles", "rnn_tiles_x3"):
        for fused in (False, True):
            pt = post_train(env, num_episodes=1, max_ep_len=5, inf_print=False, fused=fused, policy_kernel=kernel)
            with pytest.raises(ValueError, match="policy_kernel"):
                pt.policy_test(policy=mlp)
    env.close()
