"""The kernel policy step of trainer and evaluator (rvo3d_amd.policy.KernelPolicyStep) against the same launches made by
hand, bit for bit, in each of its five kinds: "mlp", "mlp_x3" (one launch), "rnn0", "rnn_tiles", "rnn_tiles_x3" (three).
The trainer tests of those modes compare the stored values with the modules within tolerances; here every stored
act / logp / val of two rollouts - the second from plans repacked after an update() - is compared as int32 with what the
entry points return when this file calls them itself, on buffers of its own, for the slot's observation, the trainer's
seed and the slot's noise step.

World: a crossing scene (every drone flies through the centre) of E x N = 11 x 37 = 407 rows: seven 64-row chunks of
the MLP kernels and thirteen 32-row tiles, the last of each ragged.  The tests assert that over the eight slots of the
two rollouts some rows have ONE velocity-obstacle row and some have SEVERAL - otherwise the rows and tiles kernels had
not every kind of work to do.  3 x 37 does not give that: run on the GPU, tight rings of 37 drones with 3 to 7 envs
had 12 to 21 rows with one VO row in the eight slots and none with several (a second neighbour on collision course
within the 2 s horizon is a 1-in-10 event among the rows with VO rows).  The ring here is as tight as the scene allows
(radius 2 +- 1 m, starts 0.6 m apart); stepped on the CPU oracle with random accelerations of the untrained policies'
scale, ten seeds each, 11 envs were the fewest (of 5, 7, ..., 15) at which every seed had at least three such rows."""
import ctypes as C
import functools

import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, _lib, crossing_world
from rvo3d_amd.policy import mlp_ac, multi_ppo
from test_gpu_rnn_tiles import _ac, _p, _stream
from test_gpu_rnn_tiles_x3 import _three_launches

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, N, T = 11, 37, 4
# kind -> (trainer arguments, precision of its plans)
KINDS = {"mlp": (dict(amp=True), "bf16"),
         "mlp_x3": (dict(amp=False, fused_mlp_fp32=True), "x3"),
         "rnn0": (dict(amp=True), "bf16"),
         "rnn_tiles": (dict(amp=True, fused_rnn_tiles=True), "bf16"),
         "rnn_tiles_x3": (dict(amp=False, fused_rnn_fp32=True), "x3")}


def _world(e=E, n=N):
    return crossing_world(e, n, (12, 12, 6), radius=2.0, radius_jitter=1.0, alt_spread=0.5, min_sep=0.6, seed=4)


def _outputs(rows):
    return [torch.empty(s, device=DEV) for s in ((rows, 3), (rows,), (rows,))]


def _mlp_sample(ac, precision, env, obs, cnt, seed, step):
    """The one launch of the MLP kinds, as test_kernel_policy_in_both_loops makes it."""
    L, rows = _lib.lib(), obs.shape[0]
    mb = ac.mlp_blob(precision)
    fn = L.rvo3d_policy_mlp_sample if precision == "bf16" else L.rvo3d_policy_mlp_x3_sample
    out = _outputs(rows)
    _lib.check(fn(_p(mb["blob"]), env.W, _p(obs), env.W, rows, _p(cnt), 12, 9, 1 if mb["tanh"] else 0, _p(ac.log_std),
                  1.0, seed, step, *[_p(x) for x in out], None, None, _stream()), "policy sample")
    torch.cuda.synchronize()
    return out


def _rows_launches(ac, env, obs, cnt, seed, step):
    """The three launches of "rnn0": rvo3d_reader_zero_features, the collapsed layer, the listed rows one workgroup
    each (rvo3d_policy_rows on the modules' own parameters)."""
    L, rows = _lib.lib(), obs.shape[0]
    zp = ac.zero_vo_plan()
    net = zp["rows_net"]
    net.slots = (env.W - 12) // 9
    feat = torch.empty((rows, zp["width"]), device=DEV)
    lst = torch.zeros(rows, dtype=torch.int32, device=DEV)
    ctr = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = _outputs(rows)
    o = [_p(x) for x in out]
    tanh = 1 if zp["tanh"] else 0
    _lib.check(L.rvo3d_reader_zero_features(_p(obs), obs.stride(0), rows, zp["state_dim"], zp["feat_dim"], _p(zp["ln_w"]),
                                            _p(zp["ln_b"]), zp["sum_h0"], zp["sumsq_h0"], zp["eps"], _p(feat),
                                            feat.stride(0), _p(cnt), _p(lst), _p(ctr), _stream()), "zero features")
    _lib.check(L.rvo3d_policy_mlp_sample(_p(zp["blob"]), zp["width"], _p(feat), feat.stride(0), rows, None, 0, 0, tanh,
                                         _p(ac.log_std), 1.0, seed, step, *o, None, None, _stream()), "collapsed layer")
    _lib.check(L.rvo3d_policy_rows(C.byref(net), _p(obs), obs.stride(0), _p(cnt), _p(lst), _p(ctr),
                                   C.c_void_p(ctr.data_ptr() + 4), tanh, _p(ac.log_std), 1.0, seed, step, *o, _stream()),
               "policy rows")
    torch.cuda.synchronize()
    return out


def _by_hand(kind, ac, env, obs, cnt, seed, step):
    precision = KINDS[kind][1]
    if kind in ("mlp", "mlp_x3"):
        return _mlp_sample(ac, precision, env, obs, cnt, seed, step)
    if kind == "rnn0":
        return _rows_launches(ac, env, obs, cnt, seed, step)
    return _three_launches(ac, precision, env, obs, cnt, 1.0, seed, step)[0]


def _blob(kind, ac):
    precision = KINDS[kind][1]
    return (ac.mlp_blob(precision) if kind in ("mlp", "mlp_x3") else ac.zero_vo_plan(precision))["blob"]


@functools.lru_cache(maxsize=None)
def _rolled(kind, e=E, n=N):
    """Two rollouts of T steps with one update() (1 + 1 iterations) between them; after each rollout - before the
    parameters change again - every slot's launches are made by hand.  Computed once per kind, shared by the tests.
    Returns the trainer, its env and model, and per rollout and slot (step, stored [act, logp, val] as the trainer left
    them, the hand-made ones, the slot's cnt)."""
    env = BatchedDroneEnv(_world(e, n))
    rows = e * n
    torch.manual_seed(0)
    ac = mlp_ac(env.W).cuda() if kind in ("mlp", "mlp_x3") else _ac(256, True, 0)
    tr = multi_ppo(env, ac, steps_per_epoch=T, max_ep_len=9, train_pi_iters=1, train_v_iters=1, seed=3, tune_gemms=False,
                   **KINDS[kind][0])
    env.reset(); env.observe()
    slots = []
    for rollout in range(2):
        if rollout:
            before = _blob(kind, ac).clone()
            tr.update(tr.buf.get())
            assert not torch.equal(before, _blob(kind, ac))      # (the second rollout runs from repacked plans)
        if kind == "rnn0":
            tr._rnn0_dense = False      # (keep the mode under test whatever this little world's density)
        assert tr._fused_mode() == kind
        step0 = tr._acct["step"] if getattr(tr, "_acct", None) else 0
        tr.collect()
        buf = tr.buf
        for t in range(T):
            obs, cnt = buf.obs[t].view(rows, env.W), buf.cnt[t].view(rows)
            hand = _by_hand(kind, ac, env, obs, cnt, tr._sample_seed, step0 + t)
            stored = [buf.act[t].reshape(rows, 3).clone(), buf.logp[t].reshape(rows).clone(),
                      buf.val[t].reshape(rows).clone()]
            slots.append((rollout, t, step0 + t, stored, hand, cnt.clone()))
    return tr, env, ac, slots


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", list(KINDS))
def test_trainer_slots_are_the_hand_made_launches(kind):
    """Every act / logp / val the trainer stored in two rollouts around an update(), bit for bit what this file's own
    launches give for the slot's observation, seed = tr._sample_seed, step = the noise counter of that slot,
    std_factor = 1."""
    tr, env, ac, slots = _rolled(kind)
    assert len(slots) == 2 * T and [s[2] for s in slots] == list(range(2 * T))
    cnt = torch.stack([s[5] for s in slots])
    one, several = int((cnt == 1).sum()), int((cnt > 1).sum())
    print(f"{kind}: {E} x {N}, {2 * T} slots: {one} rows with one VO row, {several} with several")
    assert one > 0 and several > 0      # (the kernels for rows with VO rows had rows of both kinds to do)
    for rollout, t, step, stored, hand, _ in slots:
        for name, a, b in zip(("act", "logp", "val"), stored, hand):
            assert torch.equal(_bits(a), _bits(b)), (
                f"{kind} rollout {rollout} slot {t} (step {step}): {name} differs from the hand-made launches in "
                f"{int((_bits(a) != _bits(b)).sum())} of {a.numel()} words")


@pytest.mark.parametrize("kind", list(KINDS))
def test_launcher_reproduces_a_trainer_slot(kind):
    """A second KernelPolicyStep on the same model, built here: slot 1 of the second rollout into fresh outputs has the
    trainer's bits; the next noise step gives other actions."""
    from rvo3d_amd.policy import KernelPolicyStep
    tr, env, ac, slots = _rolled(kind)
    rows = E * N
    rollout, t, step, stored, _, _ = slots[T + 1]
    assert (rollout, t) == (1, 1)
    obs, cnt = tr.buf.obs[t].view(rows, env.W), tr.buf.cnt[t].view(rows)
    ps = KernelPolicyStep(ac, kind, env.W, rows, option="the test")
    assert ps.blob_ptr == _blob(kind, ac).data_ptr()
    out = _outputs(rows)
    ps.launch(obs, cnt, *out, 1.0, tr._sample_seed, step)
    torch.cuda.synchronize()
    for name, a, b in zip(("act", "logp", "val"), stored, out):
        assert torch.equal(_bits(a), _bits(b)), name
    again = _outputs(rows)
    ps.refresh()
    ps.launch(obs, cnt, *again, 1.0, tr._sample_seed, step + 1)
    torch.cuda.synchronize()
    assert not torch.equal(again[0], out[0])
