"""The one-launch GAE ON THE DEVICE (rvo3d_gae -> gae_kernel; gae_device; RolloutBuffer / multi_ppo with fused_gae=True).
Every comparison is exact (torch.equal / assert_array_equal): the kernel runs the reference's recurrence in float64 with
every operation rounded on its own, so it equals gae_scan_loop on finite data and the reference's own multi_PPObuf output
(tests/golden/ppo_gae.npz) bit for bit; at a path end it selects 0 instead of multiplying by 0, so - unlike both Python
scans - a non-finite reward stays inside its path."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN, load
from rvo3d_amd import BatchedDroneEnv, _lib, synthetic_world
from rvo3d_amd.policy import gae_device, gae_scan_loop, mlp_ac, multi_ppo
from rvo3d_amd.policy.multi_ppo import RolloutBuffer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (2, 3, 5), (9, 2, 65), (17, 3, 64), (33, 5, 7), (300, 2, 3), (8, 37, 33)]
COEFFS = [(0.99, 0.97), (0.99, 0.95), (1.0, 1.0), (0.0, 0.5)]


def _random(shape, seed=5):
    T, E, N = shape
    g = torch.Generator().manual_seed(seed)
    rew = torch.randn(T, E, N, generator=g) * 3
    val = torch.randn(T, E, N, generator=g) * 2
    cut = torch.rand(T, E, generator=g) < 0.2
    return rew, val, cut


def _loop(rew, val, cut, gamma, lam):
    """gae_scan_loop on CPU tensors, cut [T, E]."""
    return gae_scan_loop(rew, val, cut.bool()[:, :, None].expand_as(rew), gamma, lam)


def _device(rew, val, cut, gamma, lam):
    adv, ret = gae_device(rew.to(DEV), val.to(DEV), cut.to(DEV), gamma, lam)
    assert adv.is_cuda and adv.dtype == ret.dtype == torch.float32 and adv.shape == ret.shape == rew.shape
    return adv.cpu(), ret.cpu()


@pytest.mark.parametrize("gamma,lam", COEFFS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_step_by_step_scan(shape, gamma, lam):
    rew, val, cut = _random(shape)
    a0, r0 = _loop(rew, val, cut, gamma, lam)
    a1, r1 = _device(rew, val, cut, gamma, lam)
    assert torch.equal(a1, a0) and torch.equal(r1, r0)


@pytest.mark.parametrize("pattern", ["none", "every", "first", "last_but_one", "last_row_zero"])
def test_forced_cut_patterns(pattern):
    T, E, N = 17, 3, 64
    rew, val, cut = _random((T, E, N), seed=6)
    if pattern == "none":
        cut[:] = False
    elif pattern == "every":
        cut[:] = True
    elif pattern == "first":
        cut[:] = False; cut[0] = True
    elif pattern == "last_but_one":
        cut[:] = False; cut[T - 2] = True
    else:
        cut[T - 1] = False          # the end of the buffer ends every path, whatever its byte says
    ref_cut = cut.clone(); ref_cut[T - 1] = True
    a0, r0 = _loop(rew, val, ref_cut, 0.99, 0.97)
    a1, r1 = _device(rew, val, cut, 0.99, 0.97)
    assert torch.equal(a1, a0) and torch.equal(r1, r0)


def test_reference_fixture_bit_for_bit():
    """multi_PPObuf's own output through RolloutBuffer(fused_gae=True): every column, every step, both arrays."""
    fx = load(os.path.join(GOLDEN, "ppo_gae.npz"))
    rew, val, cut = (torch.as_tensor(fx[k]).to(DEV) for k in ("rew", "val", "cuts"))
    T, E, N = rew.shape[0], 5, 3
    buf = RolloutBuffer(T, E, N, 21, 3, DEV, float(fx["gamma"]), float(fx["lam"]), fused_gae=True)
    z = torch.zeros((E, N), device=DEV)
    for t in range(T):
        buf.store(torch.zeros((E, N, 21), device=DEV), torch.zeros((E, N), dtype=torch.int32, device=DEV),
                  torch.zeros((E, N, 3), device=DEV), z + rew[t], z + val[t], z)
        if bool(cut[t]):
            buf.finish_path(torch.ones(E, dtype=torch.bool, device=DEV))
    d = buf.get()
    assert d["shape"] == (T, E, N)
    adv, ret = d["adv"].view(T, E, N).cpu().numpy(), d["ret"].view(T, E, N).cpu().numpy()
    assert adv.dtype == fx["adv"].dtype == np.float32
    for e in range(E):
        for n in range(N):
            np.testing.assert_array_equal(adv[:, e, n], fx["adv"])
            np.testing.assert_array_equal(ret[:, e, n], fx["ret"])


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_reward_stays_inside_its_path(bad):
    rew, val, cut = _random((10, 1, 1), seed=7)
    cut[:] = False; cut[4] = True
    rew[7] = bad
    adv, ret = _device(rew, val, cut, 0.99, 0.97)
    none = torch.zeros(5, 1, dtype=torch.bool)
    a_lo, r_lo = _loop(rew[:5], val[:5], none, 0.99, 0.97)
    assert torch.equal(adv[:5], a_lo) and torch.equal(ret[:5], r_lo)
    a_hi, r_hi = _loop(rew[5:], val[5:], none, 0.99, 0.97)
    assert torch.equal(adv[8:], a_hi[3:]) and torch.equal(ret[8:], r_hi[3:])
    assert bool(torch.isfinite(a_hi[3:]).all()) and bool(torch.isfinite(a_lo).all())
    assert not bool(torch.isfinite(adv[5:8]).any()) and not bool(torch.isfinite(ret[5:8]).any())


def test_cut_encodings_agree():
    rew, val, cut = _random((33, 5, 7), seed=8)
    assert bool(cut[:-1].any())
    a0, r0 = _device(rew, val, cut, 0.99, 0.97)
    for byte in (1, 2, 255):
        a1, r1 = _device(rew, val, cut.to(torch.uint8) * byte, 0.99, 0.97)
        assert torch.equal(a1, a0) and torch.equal(r1, r0), byte


def test_writes_stay_inside_the_outputs():
    """The library called directly, adv / ret carved from the middle of sentinel-filled tensors."""
    T, E, N = 9, 2, 65
    rew, val, cut = (x.to(DEV) for x in _random((T, E, N), seed=9))
    cut = cut.to(torch.uint8)
    rew0, val0, cut0 = rew.clone(), val.clone(), cut.clone()
    n, pad, sentinel = T * E * N, 300, -12345.0
    outs = [torch.full((pad + n + pad,), sentinel, device=DEV) for _ in range(2)]
    adv, ret = (o[pad:pad + n] for o in outs)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().rvo3d_gae(p(rew), p(val), p(cut), T, E, N, 0.99, 0.97, p(adv), p(ret),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rvo3d_gae")
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o[:pad] == sentinel).all()) and bool((o[pad + n:] == sentinel).all())
    assert torch.equal(rew, rew0) and torch.equal(val, val0) and torch.equal(cut, cut0)
    a0, r0 = _loop(rew.cpu(), val.cpu(), cut.cpu(), 0.99, 0.97)
    assert torch.equal(adv.view(T, E, N).cpu(), a0) and torch.equal(ret.view(T, E, N).cpu(), r0)


def test_trainer_with_fused_gae():
    world = synthetic_world(4, 8, (20, 20, 8), n_points=3, seed=4)

    def trainer(fused):
        env = BatchedDroneEnv(world)
        torch.manual_seed(0)
        tr = multi_ppo(env, mlp_ac(env.W).cuda(), steps_per_epoch=12, max_ep_len=5, amp=True, fused_gae=fused)
        env.reset(); env.observe()
        tr.collect()
        return tr

    tr = trainer(True)
    buf = tr.buf
    assert buf.fused_gae and buf.ptr == 12
    rew, val, cut = buf.rew.cpu().clone(), buf.val.cpu().clone(), buf.cut.cpu().clone()
    assert bool(cut[:-1].any())                      # a path ended inside the rollout (max_ep_len = 5 < 12)
    data = buf.get()
    a0, r0 = _loop(rew, val, cut, buf.gamma, buf.lam)
    assert torch.equal(data["adv"].cpu(), a0.reshape(-1)) and torch.equal(data["ret"].cpu(), r0.reshape(-1))
    assert buf.ptr == 0 and not bool(buf.cut.any())
    plain = trainer(False).buf.get()
    assert data.keys() == plain.keys() and data["shape"] == plain["shape"] == (12, 4, 8)
    for k, v in plain.items():
        if k != "shape":
            assert data[k].shape == v.shape and data[k].dtype == v.dtype and data[k].device == v.device, k
    stats = tr.update(data)
    assert np.isfinite(stats["kl"]) and np.isfinite(stats["loss_v"])
