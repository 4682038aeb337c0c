"""rvo3d_policy_mlp_x3_sample - config 3's policy step with split-bf16 products (float32-class) - on the GPU:
fragment layouts bit for bit on exact integer data, accuracy against a float64 forward on the env's own observations
(with the bf16 kernel failing the same bounds), the sampling tail, counts and bounds, and the trainer's "mlp_x3" mode."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, _lib, synthetic_world
from rvo3d_amd.policy import mlp_ac, multi_ppo
from test_gpu_rollout import _account_reference
from test_policy_x3_host import MU_MAX, MU_MEAN, V_REL, emulate_x3, forward64, split

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pack(ac, W, x3=True):
    L = _lib.lib()
    nbytes = L.rvo3d_policy_mlp_x3_blob_bytes if x3 else L.rvo3d_policy_mlp_blob_bytes
    pack = L.rvo3d_policy_mlp_x3_pack if x3 else L.rvo3d_policy_mlp_pack
    blob = torch.zeros(int(nbytes(W)), dtype=torch.uint8, device=DEV)
    keep = [t.detach().float().contiguous() for net in (ac.pi_net, ac.v_net) for m in net
            if isinstance(m, torch.nn.Linear) for t in (m.weight, m.bias)]
    a, b = _lib.MlpWeights(*[t.data_ptr() for t in keep[:6]]), _lib.MlpWeights(*[t.data_ptr() for t in keep[6:]])
    _lib.check(pack(C.byref(a), C.byref(b), W, _p(blob), None), "pack")
    torch.cuda.synchronize()
    return blob


def _run(blob, W, x, log_std, tanh=True, seed=7, step=0, std_factor=1.0, rows=None, cnt=None, x3=True):
    L = _lib.lib()
    rows = x.shape[0] if rows is None else rows
    out = [torch.full(s, 9.0, device=DEV) for s in ((rows, 3), (rows,), (rows,), (rows, 3), (rows, 3))]
    fn = L.rvo3d_policy_mlp_x3_sample if x3 else L.rvo3d_policy_mlp_sample
    _lib.check(fn(_p(blob), W, _p(x), x.stride(0), rows, _p(cnt), 12, 9, 1 if tanh else 0, _p(log_std), std_factor,
                  seed, step, *[_p(t) for t in out], C.c_void_p(torch.cuda.current_stream().cuda_stream)), "sample")
    torch.cuda.synchronize()
    return out  # act, logp, val, mu, raw


# ---- 1. layouts, exactly --------------------------------------------------------------------------------------------
def _exact_case(W, rows, seed, flip):
    """Integer data on which every kept product and every partial sum is exact in float32 and every dropped lo x lo
    term is zero.  Each layer's input features are split in two sets: on P the weights carry lo parts (odd integers in
    [257, 511]: 9 significant bits) against bf16-exact activations, on Q the activations carry them against small
    bf16-exact weights.  The units of the next layer's P set are computed from P inputs with small weights only (so
    they stay small integers: bf16-exact); `flip` swaps the two sets of every layer."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    sparse = lambda shape, p: (torch.rand(shape, generator=g) < p).double()
    longi = lambda shape: ri(257, 511, shape) * (ri(0, 1, shape) * 2 - 1)
    P = [torch.rand(n, generator=g) < 0.5 for n in (W, 256, 256)]
    if flip:
        P = [~p for p in P]
    P1, P2, P3 = [p.double() for p in P]
    x = ri(-1, 1, (rows, W)) * P1 + longi((rows, W)) * (1 - P1)
    x *= sparse((rows, W), 0.15)

    def layer(n_out, n_in, Pin, Pout, dens):
        # rows of Pout (small results): small weights on Pin only; other rows: long weights on Pin, small ones on Qin
        small = ri(-1, 1, (n_out, n_in)) * sparse((n_out, n_in), dens)
        long_ = longi((n_out, n_in)) * sparse((n_out, n_in), dens)
        out_p = Pout[:, None] if Pout is not None else torch.zeros((n_out, 1), dtype=torch.float64)
        return out_p * small * Pin[None, :] + (1 - out_p) * (long_ * Pin[None, :] + small * (1 - Pin[None, :]))

    ac = mlp_ac(W)
    lin = [[m for m in net if isinstance(m, torch.nn.Linear)] for net in (ac.pi_net, ac.v_net)]
    with torch.no_grad():
        for ls in lin:
            ls[0].weight.copy_(layer(256, W, P1, P2, 0.15))
            ls[0].bias.copy_(ri(-3, 3, (256,)) * P2 + longi((256,)) * (1 - P2))   # (the bias column: a P feature)
            ls[1].weight.copy_(layer(256, 256, P2, P3, 0.04))
            ls[1].bias.copy_(ri(-3, 3, (256,)))
            n3 = ls[2].out_features
            ls[2].weight.copy_(layer(n3, 256, P3, None, 0.1))
            ls[2].bias.copy_(ri(-99, 99, (n3,)))
    xf = x.float()
    with torch.no_grad():
        for ls, net in zip(lin, (ac.pi_net, ac.v_net)):
            # every partial sum below 2^24 (a bound on |W| |x| per layer), and the emulated kernel IS the float64 forward
            h = xf.double().abs()
            for i, m in enumerate(ls):
                h = h @ m.weight.double().abs().T + m.bias.double().abs()
                assert float(h.max()) < 2 ** 24
            assert torch.equal(emulate_x3(net, xf).double(), forward64(net, xf))
            # the lo parts do matter: the bf16 hi parts alone give other numbers
            assert float(split(m.weight)[1].abs().sum()) > 0
    return ac.to(DEV), xf.to(DEV)


@pytest.mark.parametrize("W", [1, 20, 40, 57, 70, 90, 102, 126])   # ks1 = 1 .. 8
@pytest.mark.parametrize("flip", [False, True])
def test_x3_layouts_with_exact_integer_data(W, flip):
    rows = 64 * 37 + 5 if W == 102 else 64 * 5 + 37
    ac, x = _exact_case(W, rows, seed=W + 1000 * flip, flip=flip)
    with torch.no_grad():
        mu_want, v_want = forward64(ac.pi_net, x).float(), forward64(ac.v_net, x).squeeze(-1).float()
    log_std = torch.tensor([-1.0, -0.5, -1.5], device=DEV)
    act, logp, val, mu, raw = _run(_pack(ac, W), W, x, log_std, tanh=False)
    assert torch.equal(mu, mu_want), int((mu != mu_want).sum())
    assert torch.equal(val, v_want), int((val != v_want).sum())
    n = 30 if W >= 20 else 4   # (one input column: few distinct rows)
    assert len(torch.unique(mu_want)) > n and len(torch.unique(v_want)) > n


# ---- 2. accuracy on the env's observations --------------------------------------------------------------------------
def _env_obs(nm, vo_share=0.1):
    E, N = 64, 16
    env = BatchedDroneEnv(synthetic_world(E, N, (9, 9, 5), n_points=3, seed=4), neighbors_num=nm)
    env.reset()
    obs, cnt = env.observe()
    x, c = obs.reshape(-1, env.W).clone(), cnt.reshape(-1).clone()
    for t in range(6):   # a few steps into the episode
        a = torch.rand((E, N, 3), device=DEV) * 2 - 1
        o, cc, *_ = env.step_policy(a, autoreset=True)
        x, c = torch.cat([x, o.reshape(-1, env.W)]), torch.cat([c, cc.reshape(-1)])
    env.close()
    short = int(vo_share * x.shape[0]) - int((c > 0).sum())
    if short > 0:   # fill VO rows in by hand (copied from rows that have them, or VO-like values) to reach the share
        g = torch.Generator(device=DEV).manual_seed(nm)
        empty = torch.nonzero(c == 0).squeeze(1)
        pick = empty[torch.randperm(empty.numel(), device=DEV, generator=g)[:short]]
        k = torch.randint(1, nm + 1, (short,), device=DEV, generator=g)
        vo = torch.randn((short, 9 * nm), device=DEV, generator=g) * 3
        x[pick, 12:] = vo * (torch.arange(9 * nm, device=DEV)[None, :] < 9 * k[:, None])
        c[pick] = k.int()
    assert float((c > 0).float().mean()) >= vo_share - 1e-3
    return x.contiguous(), c.int().contiguous()


@pytest.mark.parametrize("W", [12 + 9 * 3, 12 + 9 * 5, 12 + 9 * 10, 126])
def test_x3_accuracy_against_float64(W):
    nm = (min(W, 120) - 12) // 9
    x, cnt = _env_obs(nm)
    if W > x.shape[1]:   # the widest input the kernel takes: six more columns of VO-like data
        x = torch.cat([x, x[:, 12:12 + W - x.shape[1]]], 1).contiguous()
        cnt = None
    torch.manual_seed(W)
    ac = mlp_ac(W).to(DEV)
    log_std = ac.log_std.detach()
    with torch.no_grad():
        z64, v64 = forward64(ac.pi_net, x), forward64(ac.v_net, x).squeeze(-1)
    for x3 in (True, False):
        _, _, val, mu, _ = _run(_pack(ac, W, x3=x3), W, x, log_std, tanh=False, cnt=cnt, x3=x3)
        d_mu, d_v = (mu.double() - z64).abs(), (val.double() - v64).abs()
        ok = (float(d_mu.max()) <= MU_MAX and float(d_mu.mean()) <= MU_MEAN
              and bool((d_v <= V_REL * v64.abs().clamp(min=1.0)).all()))
        print(f"W {W} {'x3' if x3 else 'bf16'}: mu max {float(d_mu.max()):.2e} mean {float(d_mu.mean()):.2e}, "
              f"v max {float(d_v.max()):.2e}")
        if x3:
            assert ok, (float(d_mu.max()), float(d_mu.mean()), float(d_v.max()))
        else:   # the bf16 kernel on the same data: visibly outside
            assert not ok and max(float(d_mu.max()), float(d_v.max())) > 1e-3


# ---- 3. sampling ----------------------------------------------------------------------------------------------------
def test_x3_sampling_tail():
    W, rows = 102, 20000
    torch.manual_seed(3)
    ac = mlp_ac(W).to(DEV)
    x = torch.randn((rows, W), device=DEV) * 2
    log_std = torch.tensor([-1.0, -0.5, -1.5], device=DEV)
    blob = _pack(ac, W)
    L = _lib.lib()
    for sf in (1.0, 0.3):
        act, logp, val, mu, raw = _run(blob, W, x, log_std, seed=11, step=5, std_factor=sf)
        std = torch.clamp(sf * torch.exp(log_std) + 1e-6, 1e-4, 10.0)
        eps = (raw - mu) / std
        # the same noise as rvo3d_policy_sample in direct mode (mu = 0, std as here)
        zero = torch.zeros((rows, 3), device=DEV)
        out = [torch.zeros(s, device=DEV) for s in ((rows, 3), (rows,), (rows,), (rows, 3), (rows, 3))]
        hd = _lib.PolicyHeads(zero.data_ptr(), zero.data_ptr(), 3, 3, _lib.RVO3D_F32, 0, 0, 0, None, None, None, None,
                              log_std.data_ptr())
        _lib.check(L.rvo3d_policy_sample(C.byref(hd), rows, sf, 11, 5, *[_p(t) for t in out], None), "sample")
        torch.cuda.synchronize()
        assert float((raw - mu - out[4]).abs().max()) <= 1e-6    # eps * std: the same noise
        assert float((eps - out[4] / std).abs().max()) <= 2e-5
        # std_factor as in the bf16 kernel: the same std, the same noise
        blob_b = _pack(ac, W, x3=False)
        _, _, _, mu_b, raw_b = _run(blob_b, W, x, log_std, seed=11, step=5, std_factor=sf, x3=False)
        assert float((raw_b - mu_b - (raw - mu)).abs().max()) <= 1e-6
        assert np.array_equal(act.cpu().numpy(), np.round(raw.cpu().numpy(), 2))   # rint(a * 100) / 100 in float32
        lp_ref = torch.distributions.Normal(mu.double(), std.double()).log_prob(raw.double()).sum(-1)
        assert torch.allclose(logp.double(), lp_ref, atol=1e-5, rtol=1e-5), float((logp - lp_ref).abs().max())
        e = eps.cpu().numpy()
        assert abs(e.mean()) < 4 / math.sqrt(e.size) and abs(e.var() - 1) < 6 * math.sqrt(2 / e.size)
    assert not torch.equal(raw, _run(blob, W, x, log_std, seed=11, step=6, std_factor=0.3)[4])
    assert not torch.equal(raw, _run(blob, W, x, log_std, seed=12, step=5, std_factor=0.3)[4])
    assert torch.equal(raw, _run(blob, W, x, log_std, seed=11, step=5, std_factor=0.3)[4])


# ---- 4. counts and bounds -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nm", [10, 5, 3, 12])
def test_x3_counts_are_bit_identical_to_none(nm):
    W, rows = 12 + 9 * nm, 64 * 50 + 17
    g = torch.Generator(device=DEV).manual_seed(nm)
    ac = mlp_ac(W).to(DEV)
    cnt = torch.randint(0, 3, (rows,), device=DEV, generator=g, dtype=torch.int32)
    cnt[torch.rand(rows, device=DEV, generator=g) < 0.02] = nm
    cnt[64 * 7:64 * 9] = torch.randint(0, nm + 1, (128,), device=DEV, generator=g, dtype=torch.int32)
    cnt[64 * 20:64 * 21] = nm
    cnt[64 * 30:64 * 32] = 0
    x = torch.randn((rows, W), device=DEV, generator=g) * 3
    x *= (torch.arange(W, device=DEV)[None, :] < (12 + 9 * cnt.long())[:, None]).float()
    log_std = torch.tensor([-1.0, -0.5, -1.5], device=DEV)
    blob = _pack(ac, W)
    dense = _run(blob, W, x, log_std)
    sparse = _run(blob, W, x, log_std, cnt=cnt)
    for a, b in zip(dense, sparse):
        assert torch.equal(a, b)


def test_x3_reads_only_the_callers_bytes_and_rejects_bad_arguments():
    L = _lib.lib()
    W, rows = 102, 200
    ac = mlp_ac(W).to(DEV)
    blob = _pack(ac, W)
    log_std = torch.zeros(3, device=DEV)
    big = torch.full((rows * W + 64,), float("nan"), device=DEV)
    x = big[:rows * W].view(rows, W)
    x.copy_(torch.randn((rows, W), device=DEV))
    a = _run(blob, W, x, log_std)
    b = _run(blob, W, x.clone(), log_std)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and bool(torch.isfinite(a[3]).all())
    # 77 rows ending flush with the NaN tail: no byte past them is read
    tail = big[(rows - 77) * W:(rows - 77) * W + 77 * W].view(77, W)
    c = _run(blob, W, tail, log_std, rows=77)
    d = _run(blob, W, tail.clone(), log_std, rows=77)
    assert all(torch.equal(p, q) for p, q in zip(c, d)) and bool(torch.isfinite(c[3]).all())
    v = torch.zeros(8, device=DEV)
    args = lambda **k: [k.get("blob", _p(blob)), k.get("W", W), _p(x), k.get("ld", W), k.get("rows", rows), None, 12, 9,
                        1, _p(log_std), 1.0, 0, 0, _p(v), _p(v), _p(v), None, None, None]
    f = L.rvo3d_policy_mlp_x3_sample
    assert f(*args(W=127)) == -1 and b"obs_width" in L.rvo3d_last_error()
    assert f(*args(ld=W - 1)) == -1 and b"obs_ld" in L.rvo3d_last_error()
    assert f(*args(blob=C.c_void_p(blob.data_ptr() + 4))) == -1 and b"aligned" in L.rvo3d_last_error()
    assert f(*args(rows=-1)) == -1 and b"rows" in L.rvo3d_last_error()
    assert f(*args(blob=None)) == -1
    assert f(*args(rows=0)) == 0
    assert L.rvo3d_policy_mlp_x3_blob_bytes(127) == -1 and L.rvo3d_policy_mlp_x3_blob_bytes(0) == -1
    assert L.rvo3d_policy_mlp_x3_blob_bytes(102) == 2 * (7 * 16384 + 131072 + 1024 + 4096 + 131072 + 16)


# ---- 5. the trainer -------------------------------------------------------------------------------------------------
def _account_replay(world, buf, T, max_ep_len, mean_ret):
    """tests/test_gpu_rollout.py's faithful-rollout check: a second env stepped with the STORED actions reproduces every
    stored reward, cut, observation and count."""
    E, N = buf.obs.shape[1], buf.obs.shape[2]
    env2 = BatchedDroneEnv(world)
    env2.reset(); o, c = env2.observe()
    assert torch.equal(o, buf.obs[0]) and torch.equal(c, buf.cnt[0])
    ep_len = torch.zeros((E, N), dtype=torch.int32, device=DEV)
    ep_ret = torch.zeros((E, N), device=DEV)
    ret_sum = ret_n = 0.0
    for t in range(T):
        o, c, rew, done, info, fin = env2.step_policy(buf.act[t], autoreset=True)
        want = _account_reference(rew, done, fin, ep_ret, ep_len, 1, max_ep_len, t == T - 1)
        ep_ret, ep_len = want[1], want[2]
        ret_sum += want[5]; ret_n += want[6]
        assert torch.equal(torch.nan_to_num(buf.rew[t], nan=-7.0), torch.nan_to_num(want[0], nan=-7.0)), t
        assert torch.equal(buf.cut[t], want[3]), t
        if bool(want[4].any()):
            env2.reset_drones(want[4]); o, c = env2.observe()
        assert torch.equal(torch.nan_to_num(o, nan=-7.0), torch.nan_to_num(buf.obs[t + 1], nan=-7.0)), t
        assert torch.equal(c, buf.cnt[t + 1]), t
    assert mean_ret == pytest.approx(ret_sum / max(ret_n, 1.0), rel=1e-9, abs=1e-9)
    env2.close()


def test_trainer_mlp_x3_mode_is_a_faithful_float32_rollout():
    E, N, T = 64, 16, 24
    world = synthetic_world(E, N, (9, 9, 5), n_points=3, seed=4)
    env = BatchedDroneEnv(world)
    torch.manual_seed(0)
    ac = mlp_ac(env.W).cuda()
    assert multi_ppo(env, ac, steps_per_epoch=T, amp=False)._fused_mode() == "heads"
    tr = multi_ppo(env, ac, steps_per_epoch=T, max_ep_len=9, train_pi_iters=2, train_v_iters=2, amp=False, seed=3,
                   fused_mlp_fp32=True)
    assert tr._fused_mode() == "mlp_x3"
    env.reset(); env.observe()
    mean_ret = tr.collect()
    buf = tr.buf
    assert buf.ptr == T
    _account_replay(world, buf, T, 9, mean_ret)
    with torch.no_grad():
        x = buf.obs[:T].reshape(-1, env.W)
        d, _ = ac.pi(x)
        v = ac.v(x)
    assert torch.allclose(buf.val.reshape(-1), v, atol=1e-4, rtol=1e-4), float((buf.val.reshape(-1) - v).abs().max())
    z = (buf.act.reshape(-1, 3) - d.mean) / d.stddev
    assert abs(float(z.mean())) < 0.02 and abs(float(z.var()) - 1) < 0.05
    # an update changes the weights; the next rollout runs on the repacked blob
    blob0 = ac.mlp_blob("x3")["blob"].clone()
    st = tr.update(buf.get())
    assert np.isfinite(st["loss_v"])
    assert not torch.equal(blob0, ac.mlp_blob("x3")["blob"])
    tr.buf.ptr = 0
    tr.collect()
    with torch.no_grad():
        v2 = ac.v(tr.buf.obs[:T].reshape(-1, env.W))
    assert torch.allclose(tr.buf.val.reshape(-1), v2, atol=1e-4, rtol=1e-4), float((tr.buf.val.reshape(-1) - v2).abs().max())
    env.close()
