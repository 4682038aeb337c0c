"""rvo3d_policy_rnn_tiles: the biGRU actor-critic's policy step for the rows WITH velocity-obstacle rows in 32-row MFMA
tiles (csrc/rvo3d_policy_rnn_tiles.hpp), and the trainer mode built on it (multi_ppo(fused_rnn_tiles=True), "rnn_tiles").
Checked against the modules' own float32 forward (bf16-class bounds, and no worse than twice the library-GEMM "heads"
path on the same rows), for isolation between rows (list order, tile mates, unlisted rows, the list protocol), for its
sampling (bit-identical to rvo3d_policy_sample fed the kernel's own mu / v) and as a rollout: replaying the stored
actions reproduces the buffer bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, _lib, crossing_world, synthetic_world
from rvo3d_amd.policy import multi_ppo, rnn_ac
from test_gpu_rollout import _account_reference  # (the rollout bookkeeping's plain statement)

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Space:
    shape = (3,)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ac(hidden, bi, seed, mode=None):
    torch.manual_seed(seed)
    ac = rnn_ac(None, Space(), 12, 9, hidden, (256, 256), (256, 256), torch.nn.ReLU, torch.nn.Tanh, torch.nn.Identity,
                use_gpu=False, rnn_mode=mode or ("biGRU" if bi else "GRU")).cuda()
    with torch.no_grad():  # (a reader whose state moves: the default initialisation is nearly linear)
        for p_ in ac.pi.rnn_reader.parameters():
            p_.add_(torch.randn_like(p_) * 0.2)
    return ac


def _rows(rows, nm, n_list, seed):
    """obs [rows, 12 + 9 nm] with counts 1..nm (every count present among the listed rows), zeros behind each row's
    VO rows; `pick`: n_list scattered rows."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    W = 12 + 9 * nm
    cnt = torch.randint(0, nm + 1, (rows,), device=DEV, generator=g, dtype=torch.int32)
    pick = torch.randperm(rows, device=DEV, generator=g)[:n_list]
    cnt[pick] = (torch.arange(n_list, device=DEV, dtype=torch.int32) % nm) + 1
    obs = torch.randn((rows, W), device=DEV, generator=g)
    obs[:, :12] *= torch.tensor([3., 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], device=DEV)
    obs *= (torch.arange(W, device=DEV)[None, :] < (12 + 9 * cnt.long())[:, None]).float()
    return obs, cnt, pick


class Tiles:
    """One set of buffers for rvo3d_policy_rnn_tiles over `rows` observation rows."""

    def __init__(self, ac, rows, nm):
        self.tb = ac.rnn_tiles_blob()
        assert self.tb is not None
        self.rows, self.nm = rows, nm
        L = _lib.lib()
        self.work = torch.zeros(int(L.rvo3d_policy_rnn_tiles_work_bytes(rows, nm)) // 4, dtype=torch.int32, device=DEV)
        self.lst = torch.zeros(rows, dtype=torch.int32, device=DEV)
        self.ctr = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.log_std = ac.log_std.detach()

    def __call__(self, obs, cnt, listed, seed=7, step=3):
        L, tb, rows = _lib.lib(), self.tb, self.rows
        n = int(listed.numel())
        self.lst[:n] = listed.to(torch.int32)
        self.ctr[0] = n
        act = torch.full((rows, 3), 9.0, device=DEV)
        logp = torch.full((rows,), 9.0, device=DEV)
        val = torch.full((rows,), 9.0, device=DEV)
        mu = torch.full((rows, 3), 9.0, device=DEV)
        _lib.check(L.rvo3d_policy_rnn_tiles(
            _p(tb["blob"]), tb["blob_bytes"], tb["hidden"], tb["in_dim"], tb["state_dim"], tb["bidir"], _p(obs),
            obs.stride(0), _p(cnt), _p(self.lst), _p(self.ctr), C.c_void_p(self.ctr.data_ptr() + 4), _p(self.work),
            rows, self.nm, 1 if tb["tanh"] else 0, _p(self.log_std), 1.0, seed, step, _p(act), _p(logp), _p(val), _p(mu),
            _stream()), "rvo3d_policy_rnn_tiles")
        torch.cuda.synchronize()
        return act, logp, val, mu


def _heads_path(ac, obs, cnt):
    """mu / v of the library-GEMM "heads" path in bf16 (rnn_ac.prepare_input + hidden_pair + rvo3d_policy_sample)."""
    plan = ac.fused_plan(torch.bfloat16)
    assert plan is not None
    rows = obs.shape[0]
    with torch.no_grad():
        x = ac.prepare_input(obs, cnt, plan, {})
        hp, hv = ac.hidden_pair(x, plan)
    act = torch.empty((rows, 3), device=DEV); logp = torch.empty(rows, device=DEV)
    val = torch.empty(rows, device=DEV); mu = torch.empty((rows, 3), device=DEV)
    hd = _lib.PolicyHeads(hp.data_ptr(), hv.data_ptr(), hp.stride(0), hv.stride(0), _lib.RVO3D_BF16, plan["hidden"],
                          1 if plan["tanh"] else 0, 0, plan["w_pi"].data_ptr(), plan["b_pi"].data_ptr(),
                          plan["w_v"].data_ptr(), plan["b_v"].data_ptr(), ac.log_std.data_ptr())
    _lib.check(_lib.lib().rvo3d_policy_sample(C.byref(hd), rows, 1.0, 7, 3, _p(act), _p(logp), _p(val), _p(mu), None,
                                              _stream()), "rvo3d_policy_sample")
    torch.cuda.synchronize()
    return mu, val


@pytest.mark.parametrize("hidden,bi", [(256, True), (256, False), (64, True), (64, False)])
def test_rnn_tiles_matches_the_modules(hidden, bi):
    """mu (dbg_mu) and v of every listed row against the modules' float32 forward: within 3e-2 abs + rel (bf16 operands,
    as the amp rollout test allows) and at most twice the error of the "heads" bf16 path on the same rows."""
    nm, rows = 12, 3001
    ac = _ac(hidden, bi, 5 + hidden + bi)
    obs, cnt, pick = _rows(rows, nm, 997, 11)     # (997 listed rows: the last tile of most counts is ragged)
    run = Tiles(ac, rows, nm)
    act, logp, val, mu = run(obs, cnt, pick)
    with torch.no_grad():
        arg = (obs[pick], cnt[pick])
        d, _ = ac.pi(arg)
        v = ac.v(arg)
    assert torch.allclose(mu[pick], d.mean, atol=3e-2, rtol=3e-2), float((mu[pick] - d.mean).abs().max())
    assert torch.allclose(val[pick], v, atol=3e-2, rtol=3e-2), float((val[pick] - v).abs().max())
    hmu, hval = _heads_path(ac, obs[pick].contiguous(), cnt[pick].contiguous())
    e_mu, e_v = float((mu[pick] - d.mean).abs().max()), float((val[pick] - v).abs().max())
    h_mu, h_v = float((hmu - d.mean).abs().max()), float((hval - v).abs().max())
    assert e_mu <= 2 * h_mu and e_v <= 2 * h_v, (e_mu, h_mu, e_v, h_v)
    # every count 1..nm was listed; the unlisted rows keep their sentinels
    assert sorted(set(cnt[pick].tolist())) == list(range(1, nm + 1))
    untouched = torch.ones(rows, dtype=torch.bool, device=DEV)
    untouched[pick] = False
    for t in (act, logp, val, mu):
        assert bool((t[untouched] == 9.0).all())
        assert bool(torch.isfinite(t[pick]).all())


@pytest.mark.parametrize("hidden", [256, 64])
def test_rnn_tiles_isolation_and_list_protocol(hidden):
    """A row's outputs do not depend on the list's order or on its tile mates (bit for bit); count, the finished-workgroups
    word and the work area's cursors are zero after every call, and a second call with a fresh list works."""
    nm, rows = 10, 2000
    ac = _ac(hidden, True, 21)
    obs, cnt, pick = _rows(rows, nm, 700, 12)
    run = Tiles(ac, rows, nm)
    ref = run(obs, cnt, pick)
    assert run.ctr.tolist() == [0, 0] and int(run.work[:32].abs().sum()) == 0
    perm = pick[torch.randperm(pick.numel(), device=DEV)]
    got = run(obs, cnt, perm)
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    # the rows of one count alone, and that count mixed with rows of every other count: the same bits per row
    for k in (1, 2, nm):
        sub = pick[cnt[pick] == k]
        alone = run(obs, cnt, sub)
        for a, b in zip(ref, alone):
            assert torch.equal(a[sub], b[sub])
            others = torch.ones(rows, dtype=torch.bool, device=DEV)
            others[sub] = False
            assert bool((b[others] == 9.0).all())
        assert run.ctr.tolist() == [0, 0] and int(run.work[:32].abs().sum()) == 0
    # an empty list
    out = run(obs, cnt, pick[:0])
    assert all(bool((t == 9.0).all()) for t in out) and run.ctr.tolist() == [0, 0]


def test_rnn_tiles_sampling_is_rvo3d_policy_sample():
    """act / logp of the listed rows are bit-identical to rvo3d_policy_sample in direct mode (hidden 0) fed the kernel's
    own mu and v: the same Philox counter (row, step), the same tail."""
    nm, rows = 10, 1500
    ac = _ac(256, True, 31)
    obs, cnt, pick = _rows(rows, nm, 500, 13)
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


def test_rnn_tiles_blob_cache_and_bad_shapes():
    """rnn_tiles_blob: one cache entry, repacked after a parameter changes; a blob used with another shape is refused
    without a launch."""
    ac = _ac(64, True, 41)
    tb = ac.rnn_tiles_blob()
    assert ac.rnn_tiles_blob() is tb
    with torch.no_grad():
        ac.pi.net_out[0].bias.add_(1.0)
    tb2 = ac.rnn_tiles_blob()
    assert tb2 is not tb and tb2["blob"].data_ptr() == tb["blob"].data_ptr()
    assert _ac(64, True, 41, mode="LSTM").rnn_tiles_blob() is None
    L = _lib.lib()
    rows, nm = 64, 4
    obs, cnt, pick = _rows(rows, nm, 10, 1)
    run = Tiles(ac, rows, nm)
    o = torch.zeros(rows * 5, device=DEV)
    args = lambda hidden, bidir: (_p(tb2["blob"]), tb2["blob_bytes"], hidden, 9, 12, bidir, _p(obs), obs.stride(0),
                                  _p(cnt), _p(run.lst), _p(run.ctr), C.c_void_p(run.ctr.data_ptr() + 4), _p(run.work),
                                  rows, nm, 1, _p(run.log_std), 1.0, 7, 0, _p(o), _p(o), _p(o), None, None)
    assert L.rvo3d_policy_rnn_tiles(*args(256, 1)) == -1 and b"another" in L.rvo3d_last_error()
    assert L.rvo3d_policy_rnn_tiles(*args(64, 0)) == -1
    assert L.rvo3d_policy_rnn_tiles(*args(64, 1)) == 0     # (the list is empty: nothing to do)
    torch.cuda.synchronize()


def _trainer_rollout(world, T, ac):
    env = BatchedDroneEnv(world)
    tr = multi_ppo(env, ac, steps_per_epoch=T, max_ep_len=9, train_pi_iters=1, train_v_iters=1, amp=True, seed=3,
                   fused_rnn_tiles=True)
    assert tr._fused_mode() == "rnn_tiles"
    env.reset(); env.observe()
    tr.collect()
    return env, tr


@pytest.mark.parametrize("world_kind", ["dense", "crossing"])
def test_rnn_tiles_rollout_is_a_faithful_rollout(world_kind):
    """multi_ppo(amp=True, fused_rnn_tiles=True) with the trained architecture (biGRU 256, (256, 256) heads): the mode is
    "rnn_tiles" and stays so after a dense rollout; replaying the stored actions reproduces obs, counts and rewards bit
    for bit; values within 3e-2 of the module, the stored log-probabilities consistent with the module's distribution;
    update() runs."""
    E, N, T = 64, 16, 24
    world = synthetic_world(E, N, (9, 9, 5), n_points=3, seed=4) if world_kind == "dense" else \
        crossing_world(E, N, (12, 12, 6), radius=4.0, alt_spread=0.5, seed=4)
    ac = _ac(256, True, 0)
    env, tr = _trainer_rollout(world, T, ac)
    buf = tr.buf
    frac = float((buf.cnt[:T] > 0).float().mean())
    # the kernel had rows to do (the dense world: more than 1 in 1000 - "rnn0" leaves for "heads" above 1 in 500)
    assert frac > (1e-3 if world_kind == "dense" else 0.0), frac
    tr.collect()
    assert tr._fused_mode() == "rnn_tiles"        # (no density switch)
    env, tr = _trainer_rollout(world, T, ac)      # (a fresh rollout from the reset state for the replay below)
    buf = tr.buf
    env2 = BatchedDroneEnv(world)
    env2.reset(); o, c = env2.observe()
    assert torch.equal(o, buf.obs[0]) and torch.equal(c, buf.cnt[0])
    ep_len = torch.zeros((E, N), dtype=torch.int32, device=DEV)
    ep_ret = torch.zeros((E, N), device=DEV)
    for t in range(T):
        o, c, rew, done, info, fin = env2.step_policy(buf.act[t], autoreset=True)
        want = _account_reference(rew, done, fin, ep_ret, ep_len, 1, 9, t == T - 1)
        ep_ret, ep_len = want[1], want[2]
        assert torch.equal(torch.nan_to_num(buf.rew[t], nan=-7.0), torch.nan_to_num(want[0], nan=-7.0)), t
        if bool(want[4].any()):
            env2.reset_drones(want[4]); o, c = env2.observe()
        assert torch.equal(torch.nan_to_num(o, nan=-7.0), torch.nan_to_num(buf.obs[t + 1], nan=-7.0)), t
        assert torch.equal(c, buf.cnt[t + 1]), t
    with torch.no_grad():
        x = buf.obs[:T].reshape(-1, env.W)
        arg = (x, buf.cnt[:T].reshape(-1))
        d, _ = ac.pi(arg)
        v = ac.v(arg)
    assert torch.allclose(buf.val[:T].reshape(-1), v, atol=3e-2, rtol=3e-2)
    lp_of_stored = d.log_prob(buf.act[:T].reshape(-1, 3)).sum(-1)
    assert float((buf.logp[:T].reshape(-1) - lp_of_stored).abs().mean()) < 0.12
    st = tr.update(buf.get())
    assert np.isfinite(st["loss_v"])


def test_rnn_tiles_mode_refuses_what_it_cannot_run():
    env = BatchedDroneEnv(synthetic_world(4, 8, (9, 9, 5), n_points=3, seed=4))
    with pytest.raises(ValueError):
        multi_ppo(env, _ac(256, True, 0), steps_per_epoch=4, amp=False, fused_rnn_tiles=True)
    with pytest.raises(ValueError):
        multi_ppo(env, _ac(256, True, 0, mode="LSTM"), steps_per_epoch=4, amp=True, fused_rnn_tiles=True)
    tr = multi_ppo(env, _ac(256, True, 0), steps_per_epoch=4, amp=True)
    assert tr._fused_mode() == "rnn0"          # (the flag off: what it was)
