"""CPU-side checks of the one-launch GAE (rvo3d_gae / gae_device / RolloutBuffer(fused_gae=...)): the library's argument
checks (they precede every HIP call, so they run without a GPU and on made-up addresses - nothing is dereferenced), the
Python wrapper's own checks, and that a CPU buffer ignores the flag.  The kernel itself: tests/test_gpu_gae.py."""
import pytest
import torch

from rvo3d_amd import _lib
from rvo3d_amd.policy import gae_device
from rvo3d_amd.policy.multi_ppo import RolloutBuffer

T, E, N = 4, 2, 3
N4 = T * E * N * 4                       # bytes of rew / val / adv / ret
REW, VAL, CUT, ADV, RET = 0x10000000, 0x10001000, 0x10002000, 0x10003000, 0x10004000  # made-up, disjoint


@pytest.fixture(scope="module")
def L():
    _lib.build_hip()
    return _lib.lib()


def _call(L, rew=REW, val=VAL, cut=CUT, steps=T, envs=E, drones=N, gamma=0.99, lam=0.97, adv=ADV, ret=RET):
    return L.rvo3d_gae(rew, val, cut, steps, envs, drones, gamma, lam, adv, ret, None)


@pytest.mark.parametrize("which", ["rew", "val", "cut", "adv", "ret"])
def test_null_pointer_is_rejected(L, which):
    assert _call(L, **{which: None}) == -1
    assert b"null" in L.rvo3d_last_error()


@pytest.mark.parametrize("which", ["steps", "envs", "drones"])
def test_empty_extent_is_rejected(L, which):
    assert _call(L, **{which: 0}) == -1
    assert which.encode() in L.rvo3d_last_error()


def test_non_finite_gamma_is_rejected(L):
    assert _call(L, gamma=float("nan")) == -1
    assert b"finite" in L.rvo3d_last_error()
    assert _call(L, lam=float("inf")) == -1
    assert b"finite" in L.rvo3d_last_error()


def test_output_on_an_input_is_rejected(L):
    assert _call(L, adv=REW) == -1
    assert b"overlap" in L.rvo3d_last_error()
    assert _call(L, ret=VAL + N4 - 4) == -1      # the last float of val
    assert b"overlap" in L.rvo3d_last_error()
    assert _call(L, adv=CUT + T * E - 1) == -1   # the last cut byte
    assert b"overlap" in L.rvo3d_last_error()


def test_ret_inside_adv_is_rejected(L):
    assert _call(L, ret=ADV + 8) == -1
    assert b"overlap" in L.rvo3d_last_error()
    assert _call(L, ret=ADV + N4 - 4) == -1
    assert b"overlap" in L.rvo3d_last_error()


def _filled(fused):
    g = torch.Generator().manual_seed(11)
    buf = RolloutBuffer(6, 2, 3, 21, 3, "cpu", 0.99, 0.97, fused_gae=fused)
    for t in range(6):
        buf.store(torch.zeros(2, 3, 21), torch.zeros(2, 3, dtype=torch.int32), torch.randn(2, 3, 3, generator=g),
                  torch.randn(2, 3, generator=g) * 3, torch.randn(2, 3, generator=g) * 2, torch.randn(2, 3, generator=g))
        if t == 2:
            buf.finish_path(torch.tensor([True, False]))
    return buf


def test_cpu_buffer_ignores_the_flag():
    a, b = _filled(True), _filled(False)
    assert a.fused_gae and not b.fused_gae
    da, db = a.get(), b.get()
    assert da.keys() == db.keys() and da["shape"] == db["shape"] == (6, 2, 3)
    for k in db:
        if k != "shape":
            assert da[k].dtype == db[k].dtype and torch.equal(da[k], db[k]), k
    assert a.ptr == 0 and not bool(a.cut.any())


def test_gae_device_checks_its_tensors():
    rew, val, cut = torch.zeros(T, E, N), torch.zeros(T, E, N), torch.zeros(T, E, dtype=torch.bool)
    with pytest.raises(ValueError, match="float32"):
        gae_device(rew.double(), val, cut)
    with pytest.raises(ValueError, match="CUDA"):
        gae_device(rew, val, cut)
    with pytest.raises(ValueError, match=r"cut \[T, E\]"):
        gae_device(rew, val, cut[:, :, None].expand(T, E, N))
    with pytest.raises(ValueError, match="bool"):
        gae_device(rew, val, cut.float())
